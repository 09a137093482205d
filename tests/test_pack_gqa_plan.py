"""CPU tests of the PackGQA routing: FA_FLAG_PACK_GQA (include/fa_fwd.h) is a hint that plan_fwd (csrc/fa_fwd_api.hip) honours
with the pk family -- `pk_fwd_kernel D=<tile> waves=4[ SOFTCAP] block_m=128 splits=<n>` -- exactly for GQA / MQA calls of 16-bit
types at head dims <= 128 without fp8, ALiBi, dropout, attention_chunk, a V head dim of its own or a qv-shaped call; every other
call is planned as without the bit.  tests/test_pack_gqa_gpu.py checks what the named kernels compute."""
import ctypes
import re

import pytest

from flash_attention_annotated_amd import _lib

ADDR = 0x10000  # an aligned dummy address: nothing is dereferenced
FP8 = _lib.FA_DTYPE_FP8_E4M3
PK = _lib.FA_FLAG_PACK_GQA


def _params(b=2, h=32, h_k=8, sq=8, sk=8192, d=128, d_v=0, dtype=_lib.FA_DTYPE_BF16, num_splits=1, **fields):
    """Dense contiguous (b, s, h, d) tensors, a dummy workspace large enough for any split or fp8 expansion; no flag."""
    dv = d_v or d
    p = _lib.new_params()
    for f in ("q", "k", "v", "o", "softmax_lse", "workspace"):
        setattr(p, f, ADDR)
    p.workspace_bytes = 1 << 40
    p.b, p.seqlen_q, p.seqlen_k, p.h, p.h_k, p.d, p.d_v, p.dtype, p.num_splits = b, sq, sk, h, h_k, d, d_v, dtype, num_splits
    for t, rows, heads, width in (("q", sq, h, d), ("k", sk, h_k, d), ("v", sk, h_k, dv), ("o", sq, h, dv)):
        setattr(p, f"{t}_head_stride", width)
        setattr(p, f"{t}_row_stride", heads * width)
        setattr(p, f"{t}_batch_stride", rows * heads * width)
    p.softmax_scale = d ** -0.5
    p.window_size_left = p.window_size_right = -1
    for k, v in fields.items():
        setattr(p, k, v)
    return p


def _plan(lib, p, flags):
    q = _lib.FaFwdParams.from_buffer_copy(p)
    q.flags = p.flags | flags
    name = lib.fa_fwd_plan_name(ctypes.byref(q), 256)
    return None if name is None else name.decode()


PAGED = dict(block_table=ADDR, page_block_size=64, block_table_batch_stride=128)
HONOURED = [  # (id, params, plan with the flag)
    ("dense", _params(), "pk_fwd_kernel D=128 waves=4 block_m=128 splits=1"),
    ("dense_d64_causal", _params(d=64, is_causal=1), "pk_fwd_kernel D=64 waves=4 block_m=128 splits=1"),
    ("dense_d96", _params(d=96), "pk_fwd_kernel D=128 waves=4 block_m=128 splits=1"),
    ("dense_softcap", _params(softcap=30.0), "pk_fwd_kernel D=128 waves=4 SOFTCAP block_m=128 splits=1"),
    ("dense_fp16_mqa", _params(h=8, h_k=1, dtype=_lib.FA_DTYPE_FP16), "pk_fwd_kernel D=128 waves=4 block_m=128 splits=1"),
    ("dense_long_q", _params(sq=4096, sk=4096, is_causal=1), "pk_fwd_kernel D=128 waves=4 block_m=128 splits=1"),
    ("fa3_window", _params(window_size_left=17, window_size_right=0, flags=_lib.FA_FLAG_FA3_WINDOW),
     "pk_fwd_kernel D=128 waves=4 block_m=128 splits=1"),
    ("varlen", _params(b=256, sq=512, sk=512, cu_seqlens_q=ADDR, cu_seqlens_k=ADDR, total_q=70000, total_k=70000),
     "pk_fwd_kernel D=128 waves=4 block_m=128 splits=1"),
    ("varlen_seqused", _params(b=5, sq=64, sk=130, cu_seqlens_q=ADDR, cu_seqlens_k=ADDR, seqused_q=ADDR, seqused_k=ADDR,
                               total_q=105, total_k=208), "pk_fwd_kernel D=128 waves=4 block_m=128 splits=1"),
    ("paged", _params(seqused_k=ADDR, **PAGED), "pk_fwd_kernel D=128 waves=4 block_m=128 splits=1"),
    ("paged_odd_page", _params(seqused_k=ADDR, block_table=ADDR, page_block_size=48, block_table_batch_stride=256),
     "pk_fwd_kernel D=128 waves=4 block_m=128 splits=1"),
    ("cache_batch_idx_leftpad", _params(seqused_k=ADDR, kv_batch_idx=ADDR, leftpad_k=ADDR),
     "pk_fwd_kernel D=128 waves=4 block_m=128 splits=1"),
    ("ragged_over_paged_cache", _params(b=64, sq=512, cu_seqlens_q=ADDR, seqused_k=ADDR, total_q=2108, **PAGED),
     "pk_fwd_kernel D=128 waves=4 block_m=128 splits=1"),
    ("ragged_over_cache_split", _params(b=5, sq=130, cu_seqlens_q=ADDR, seqused_k=ADDR, total_q=150, num_splits=3),
     "pk_fwd_kernel D=128 waves=4 block_m=128 splits=3"),
    ("split", _params(num_splits=4), "pk_fwd_kernel D=128 waves=4 block_m=128 splits=4"),
    ("split_paged_softcap", _params(num_splits=4, seqused_k=ADDR, softcap=30.0, **PAGED),
     "pk_fwd_kernel D=128 waves=4 SOFTCAP block_m=128 splits=4"),
    # num_splits = 0: groups = row blocks of packed rows x kv heads = ceil(8 * 4 / 128) * 2 batches * 8 = 16 <= 512, 128 key
    # blocks -> min(ceil(1024 / 16), 128 / 4) = 32 parts
    ("split_heuristic", _params(num_splits=0), "pk_fwd_kernel D=128 waves=4 block_m=128 splits=32"),
    # ... 256 short sequences fill the chip without a split: min(256 * 4, 70000 * 4 / 128 + 256) * 8 groups > 512
    ("split_heuristic_full", _params(b=256, sq=512, cu_seqlens_q=ADDR, seqused_k=ADDR, total_q=70000, num_splits=0),
     "pk_fwd_kernel D=128 waves=4 block_m=128 splits=1"),
    # the C-ABI knows no decode swap (the bindings fold a single-token GQA group into the rows, after which h == h_k)
    ("single_token_at_the_abi", _params(sq=1), "pk_fwd_kernel D=128 waves=4 block_m=128 splits=1"),
]


@pytest.mark.parametrize("params,name", [r[1:] for r in HONOURED], ids=[r[0] for r in HONOURED])
def test_flag_is_honoured(built_lib, params, name):
    assert built_lib.fa_fwd_validate(ctypes.byref(params)) == 0
    assert _plan(built_lib, params, PK) == name
    without = _plan(built_lib, params, 0)
    assert without is not None and not without.startswith("pk_fwd_kernel"), without


QV = dict(qv=ADDR, qv_head_stride=512, qv_row_stride=32 * 512, qv_batch_stride=8 * 32 * 512)
NOT_HONOURED = [  # (id, params): the plan with the flag is the plan without it
    ("mha", _params(h=8, h_k=8)),
    ("mha_paged_split", _params(h=8, h_k=8, num_splits=4, seqused_k=ADDR, **PAGED)),
    ("fp8", _params(dtype=FP8)),
    ("fp8_d64", _params(d=64, dtype=FP8)),
    ("alibi", _params(alibi_slopes=ADDR)),
    ("dropout", _params(p_dropout=0.1, rng_state=ADDR)),
    ("attention_chunk", _params(attention_chunk=1024)),
    ("dv_differs", _params(d=64, d_v=128)),
    ("d192_dv128", _params(d=192, d_v=128)),
    ("qv", _params(d=64, d_v=512, **QV)),
    ("qv_shaped_paged", _params(d=64, d_v=384, seqused_k=ADDR, **PAGED)),
    ("qv_shaped_split", _params(d=64, d_v=512, num_splits=3)),
    ("dv512_columns", _params(d=64, d_v=512)),
    ("d192", _params(d=192)),
    ("d256_softcap", _params(d=256, softcap=30.0)),
]


@pytest.mark.parametrize("params", [r[1] for r in NOT_HONOURED], ids=[r[0] for r in NOT_HONOURED])
def test_flag_changes_nothing_elsewhere(built_lib, params):
    assert built_lib.fa_fwd_validate(ctypes.byref(params)) == 0
    without, with_flag = _plan(built_lib, params, 0), _plan(built_lib, params, PK)
    assert without is not None and with_flag == without
    flagged = _lib.FaFwdParams.from_buffer_copy(params)
    flagged.flags |= PK
    assert built_lib.fa_fwd_workspace_size(ctypes.byref(flagged)) == built_lib.fa_fwd_workspace_size(ctypes.byref(params))


def test_plan_without_the_flag_is_unchanged(built_lib):
    """pack_gqa = None / False set no bit: the routes of the short-query shapes the flag is for stay what they were."""
    assert _plan(built_lib, _params(), 0) == "fwd_kernel D=128 waves=4 block_m=128 splits=1"
    assert _plan(built_lib, _params(seqused_k=ADDR, **PAGED), 0) == "fwd_kernel D=128 waves=8 block_m=256 splits=1"
    assert _plan(built_lib, _params(b=64, sq=512, cu_seqlens_q=ADDR, seqused_k=ADDR, total_q=2108), 0) == \
        "fwd_kernel_w64 D=128 DEFF=128 waves=4 block_m=256 splits=1"


def test_abi_is_unchanged(built_lib):
    assert built_lib.fa_abi_version() == 13 == _lib.FA_ABI_VERSION
    assert built_lib.fa_fwd_params_size() == 464 == ctypes.sizeof(_lib.FaFwdParams)
    assert PK == 4 and PK & (_lib.FA_FLAG_FA3_WINDOW | _lib.FA_FLAG_SDMASK_SIGNED) == 0


@pytest.mark.parametrize("kw", [dict(num_splits=4), dict(num_splits=3, seqused_k=ADDR, **PAGED),
                                dict(b=5, sq=130, cu_seqlens_q=ADDR, seqused_k=ADDR, total_q=150, num_splits=3)],
                         ids=["dense", "paged", "ragged"])
def test_split_workspace_is_that_of_the_unpacked_call(built_lib, kw):
    """The split partials keep the layouts the merge reads: (splits, rows, h, d) fp32 and (splits, h, rows) fp32."""
    p = _params(**kw)
    flagged = _lib.FaFwdParams.from_buffer_copy(p)
    flagged.flags |= PK
    assert _plan(built_lib, p, PK).startswith("pk_fwd_kernel ") and f" splits={kw['num_splits']}" in _plan(built_lib, p, PK)
    rows = p.total_q if p.cu_seqlens_q else p.b * p.seqlen_q
    align = lambda x: (x + 255) & ~255  # noqa: E731
    want = align(kw["num_splits"] * rows * p.h * p.d * 4) + align(kw["num_splits"] * rows * p.h * 4)
    assert built_lib.fa_fwd_workspace_size(ctypes.byref(flagged)) == built_lib.fa_fwd_workspace_size(ctypes.byref(p)) == want
    p.workspace = None  # ... and a split plan without its workspace is refused like any other
    assert _plan(built_lib, p, PK) is None


def test_grid_overflow_gives_no_plan(built_lib):
    """2^19 (batch, kv head) groups x 2^15 row blocks do not fit a 31-bit grid: no plan name, FA_ERR_BAD_SHAPE from fa_fwd --
    as for the other families (the unpacked plan of this shape overflows as well)."""
    p = _params(b=65536, sq=1 << 20, sk=64)
    assert built_lib.fa_fwd_validate(ctypes.byref(p)) == 0
    assert _plan(built_lib, p, PK) is None and _plan(built_lib, p, 0) is None
    # packed rows are counted in 32 bits: a group of 2^31 or more packed rows keeps the unpacked plan
    p = _params(b=1, h=64, h_k=1, sq=1 << 25, sk=64)
    assert _plan(built_lib, p, PK) == _plan(built_lib, p, 0) is not None


# the instantiations of fa::pk_fwd_kernel<T, D, SOFTCAP> (csrc/fa_fwd_kernel_pk.h), launched from launch_pk (csrc/fa_fwd_api.hip)
PK_KERNELS = {
    ("bf16", 64, False), ("bf16", 64, True), ("bf16", 128, False), ("bf16", 128, True),
    ("fp16", 64, False), ("fp16", 64, True), ("fp16", 128, False), ("fp16", 128, True),
}


def test_device_code_has_exactly_the_eight_instantiations():
    from device_asm import device_asm
    txt = open(device_asm("fa_fwd_api.hip")).read()
    syms = re.findall(r"^\s*\.amdhsa_kernel (\w*pk_fwd_kernel\w*)$", txt, re.M)
    assert len(syms) == len(set(syms)) == 8, syms
    got = set()
    for s in syms:
        m = re.match(r"_ZN2fa13pk_fwd_kernelI(DF16b|DF16_)Li(\d+)ELb([01])EEEvNS_8PkParamsE$", s)
        assert m, s
        got.add(({"DF16b": "bf16", "DF16_": "fp16"}[m.group(1)], int(m.group(2)), m.group(3) == "1"))
    assert got == PK_KERNELS
    # (a family of its own in tests/plan_universe.py: the names do not collide with the `fwd_kernel...` symbols)
    assert not any(re.match(r"_ZN2fa\d+fwd_kernel", s) for s in syms)
