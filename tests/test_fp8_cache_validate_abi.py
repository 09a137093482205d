"""CPU test of the validation that fa_fwd_kv8_validate and fa_fwd_qv8_validate share (csrc/fa_fwd_internal.h:
validate_fp8_cache): every defect that body owns, applied to an otherwise valid call of each route, gets the same status from
both.  The route's own shape rules are tests/test_kv8_abi.py's and tests/test_qv8_abi.py's.  Nothing here touches a device."""
import pytest

from flash_attention_annotated_amd import _lib

ADDR = 0x10000  # an aligned dummy address: nothing is dereferenced
OK, BAD_SHAPE, BAD_STRIDE, UNSUPPORTED, WORKSPACE = 0, -5, -6, -7, -11


def _params(route, **fields):
    """A valid decode call: kv8 -- q (2, 1, 8, 128) over an e4m3 cache (2, 320, 2, 128); qv8 -- q (2, 1, 16, 64), qv / o
    (2, 1, 16, 512) over K (2, 320, 1, 64), V (2, 320, 1, 512).  q / o / qv strides in 16-bit elements, k / v strides in bytes."""
    b, sq, sk = 2, 1, 320
    h, h_k, d, dv = (8, 2, 128, 128) if route == "kv8" else (16, 1, 64, 512)
    p = _lib.new_params()
    for f in ("q", "k", "v", "o", "softmax_lse", "workspace"):
        setattr(p, f, ADDR)
    p.workspace_bytes = 1 << 40
    p.b, p.seqlen_q, p.seqlen_k, p.h, p.h_k, p.d, p.dtype = b, sq, sk, h, h_k, d, _lib.FA_DTYPE_BF16
    tensors = [("q", sq, h, d), ("k", sk, h_k, d), ("v", sk, h_k, dv), ("o", sq, h, dv)]
    if route == "qv8":
        p.d_v, p.qv = dv, ADDR
        tensors.append(("qv", sq, h, dv))
    for t, rows, heads, w in tensors:
        setattr(p, f"{t}_head_stride", w)
        setattr(p, f"{t}_row_stride", heads * w)
        setattr(p, f"{t}_batch_stride", rows * heads * w)
    p.softmax_scale = 0.125
    p.window_size_left = p.window_size_right = -1
    p.num_splits = 1
    for k, v in fields.items():
        setattr(p, k, v(p) if callable(v) else v)
    return p


def _plus(field, by):
    return {field: lambda p: getattr(p, field) + by}


PAGED = dict(block_table=ADDR, page_block_size=64, block_table_batch_stride=16)
SPLIT = dict(num_splits=3)  # 320 keys = 5 blocks: three parts, so the workspace is needed

DEFECTS = [
    ("valid", {}, OK),
    ("valid_paged", PAGED, OK),
    ("valid_split", SPLIT, OK),
    # q / o strides: multiples of 8 elements
    ("q_row_stride_4", _plus("q_row_stride", 4), BAD_STRIDE),
    ("q_head_stride_4", _plus("q_head_stride", 4), BAD_STRIDE),
    ("q_batch_stride_4", _plus("q_batch_stride", 4), BAD_STRIDE),
    ("o_row_stride_4", _plus("o_row_stride", 4), BAD_STRIDE),
    ("o_head_stride_12", _plus("o_head_stride", 12), BAD_STRIDE),
    ("o_batch_stride_4", _plus("o_batch_stride", 4), BAD_STRIDE),
    # k / v strides: multiples of 16 bytes
    ("k_row_stride_8", _plus("k_row_stride", 8), BAD_STRIDE),
    ("k_head_stride_8", _plus("k_head_stride", 8), BAD_STRIDE),
    ("k_batch_stride_8", _plus("k_batch_stride", 8), BAD_STRIDE),
    ("v_row_stride_8", _plus("v_row_stride", 8), BAD_STRIDE),
    ("v_head_stride_24", _plus("v_head_stride", 24), BAD_STRIDE),
    ("v_batch_stride_8", _plus("v_batch_stride", 8), BAD_STRIDE),
    # the row stride the 32-bit lane offset multiplies
    ("k_row_stride_2_24", dict(k_row_stride=1 << 24), BAD_STRIDE),
    ("v_row_stride_2_24", dict(v_row_stride=1 << 24), BAD_STRIDE),
    ("k_row_stride_below_2_24", dict(k_row_stride=(1 << 24) - 16), OK),
    ("k_row_stride_negative", dict(k_row_stride=-16), BAD_STRIDE),
    ("v_row_stride_negative", dict(v_row_stride=-16), BAD_STRIDE),
    # 16-byte base pointers
    ("q_pointer", dict(q=ADDR + 8), BAD_STRIDE),
    ("k_pointer", dict(k=ADDR + 8), BAD_STRIDE),
    ("v_pointer", dict(v=ADDR + 4), BAD_STRIDE),
    ("o_pointer", dict(o=ADDR + 2), BAD_STRIDE),
    # descales: 32-bit non-negative strides, 4-byte pointers
    ("k_descale_batch_stride_negative", dict(k_descale=ADDR, k_descale_batch_stride=-1), BAD_STRIDE),
    ("k_descale_head_stride_wide", dict(k_descale=ADDR, k_descale_head_stride=1 << 31), BAD_STRIDE),
    ("v_descale_batch_stride_wide", dict(v_descale=ADDR, v_descale_batch_stride=1 << 31), BAD_STRIDE),
    ("v_descale_head_stride_negative", dict(v_descale=ADDR, v_descale_head_stride=-1), BAD_STRIDE),
    ("descale_stride_without_pointer", dict(k_descale_batch_stride=-1), BAD_STRIDE),
    ("k_descale_pointer", dict(k_descale=ADDR + 2), BAD_STRIDE),
    ("v_descale_pointer", dict(v_descale=ADDR + 1), BAD_STRIDE),
    ("descales", dict(k_descale=ADDR, v_descale=ADDR + 4, k_descale_batch_stride=2, v_descale_head_stride=1), OK),
    ("num_splits_negative", dict(num_splits=-1), BAD_SHAPE),
    ("softmax_scale_nan", dict(softmax_scale=float("nan")), BAD_SHAPE),
    ("softcap_nan", dict(softcap=float("nan")), BAD_SHAPE),
    ("softcap_negative", dict(softcap=-1.0), BAD_SHAPE),
    ("leftpad_with_block_table", dict(PAGED, leftpad_k=ADDR), UNSUPPORTED),
    ("block_table_with_kv_batch_idx", dict(PAGED, kv_batch_idx=ADDR), UNSUPPORTED),
    ("page_block_size_0", dict(PAGED, page_block_size=0), BAD_SHAPE),
    ("page_block_size_negative", dict(PAGED, page_block_size=-64), BAD_SHAPE),
    ("block_table_stride_negative", dict(PAGED, block_table_batch_stride=-1), BAD_STRIDE),
    ("block_table_stride_wide", dict(PAGED, block_table_batch_stride=1 << 31), BAD_STRIDE),
    ("workspace_missing", dict(SPLIT, workspace=0), WORKSPACE),
    ("workspace_misaligned", dict(SPLIT, workspace=ADDR + 128), WORKSPACE),
    ("workspace_short", dict(SPLIT, workspace_bytes=1024), WORKSPACE),
    ("workspace_unused_when_not_split", dict(workspace=0, workspace_bytes=0), OK),
    # the order of the report: strides before num_splits before the cache forms before the workspace
    ("stride_before_splits", dict(_plus("k_row_stride", 8), num_splits=-1), BAD_STRIDE),
    ("splits_before_paging", dict(PAGED, num_splits=-1, page_block_size=0), BAD_SHAPE),
    ("paging_before_workspace", dict(PAGED, num_splits=3, workspace=0, block_table_batch_stride=-1), BAD_STRIDE),
]


@pytest.mark.parametrize("name,fields,status", DEFECTS, ids=[r[0] for r in DEFECTS])
def test_shared_validate_body(name, fields, status):
    lib = _lib.load()
    kv8, qv8 = lib.fa_fwd_kv8_validate(_params("kv8", **fields)), lib.fa_fwd_qv8_validate(_params("qv8", **fields))
    assert kv8 == qv8 == status
    if status == OK:
        assert lib.fa_fwd_kv8_plan_name(_params("kv8", **fields), 256) and lib.fa_fwd_qv8_plan_name(_params("qv8", **fields), 256)


def test_exact_workspace_is_enough():
    """The workspace check takes fa_fwd_*_workspace_size's own answer, to the byte."""
    lib = _lib.load()
    for route, size, validate in (("kv8", lib.fa_fwd_kv8_workspace_size, lib.fa_fwd_kv8_validate),
                                  ("qv8", lib.fa_fwd_qv8_workspace_size, lib.fa_fwd_qv8_validate)):
        need = size(_params(route, **SPLIT))
        assert need > 0
        assert validate(_params(route, **SPLIT, workspace_bytes=need)) == OK
        assert validate(_params(route, **SPLIT, workspace_bytes=need - 1)) == WORKSPACE
