"""CPU tests of the FA3 qv surface at the C-ABI (include/fa_fwd.h, ABI v13): the qv fields of fa_fwd_params and the d_v
field of fa_kvcache_append_params in both the header and the ctypes mirror, the validation rules of the qv kernel, its
split-KV workspace, and its gfx950 ISA (no scratch).  No kernel is launched here."""
import ctypes
import os
import re
import subprocess

import pytest

from flash_attention_annotated_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _struct_fields(name):
    text = open(os.path.join(ROOT, "include", "fa_fwd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        base = re.match(r"(?:const\s+)?\w+\s*\**\s*", decl).group(0)
        for part in decl[len(base):].split(","):
            fields.append(part.strip().lstrip("*").strip())
        if fields and fields[-1] == "":
            fields.pop()
    return fields


def test_abi_v13_fields_in_header_and_mirror(built_lib):
    assert _lib.FA_ABI_VERSION == 13 and built_lib.fa_abi_version() == 13
    hdr = _struct_fields("fa_fwd_params")
    assert hdr[-4:] == ["qv", "qv_batch_stride", "qv_row_stride", "qv_head_stride"]
    assert [f[0] for f in _lib.FaFwdParams._fields_] == hdr
    app = _struct_fields("fa_kvcache_append_params")
    assert "d_v" in app
    assert [f[0] for f in _lib.FaKvcacheAppendParams._fields_] == app
    assert built_lib.fa_fwd_params_size() == ctypes.sizeof(_lib.FaFwdParams)
    assert built_lib.fa_kvcache_append_params_size() == ctypes.sizeof(_lib.FaKvcacheAppendParams)


def _mla(b=4, sq=1, h=16, h_k=1, sk=4096, d=64, dv=512):
    """MLA decode params: q (b, sq, h, d), qv (b, sq, h, dv), K and V as column views of one (b, sk, h_k, d + dv) cache."""
    p = _lib.new_params()
    for f in ("q", "k", "v", "o", "softmax_lse", "qv"):
        setattr(p, f, 0x100000)
    p.v = 0x100000 + 2 * d
    p.b, p.seqlen_q, p.seqlen_k, p.h, p.h_k, p.d, p.d_v = b, sq, sk, h, h_k, d, dv
    p.dtype = _lib.FA_DTYPE_BF16
    p.q_row_stride, p.q_head_stride, p.q_batch_stride = h * d, d, sq * h * d
    p.qv_row_stride, p.qv_head_stride, p.qv_batch_stride = h * dv, dv, sq * h * dv
    p.o_row_stride, p.o_head_stride, p.o_batch_stride = h * dv, dv, sq * h * dv
    for t in ("k", "v"):
        setattr(p, f"{t}_row_stride", h_k * (d + dv))
        setattr(p, f"{t}_head_stride", d + dv)
        setattr(p, f"{t}_batch_stride", sk * h_k * (d + dv))
    p.softmax_scale = (d + dv) ** -0.5
    p.window_size_left = p.window_size_right = -1
    p.num_splits = 1
    return p


def _with_workspace(lib, p):
    need = lib.fa_fwd_workspace_size(ctypes.byref(p))
    assert need >= 0
    if need:
        p.workspace, p.workspace_bytes = 0x10000000, need
    return need


def test_validate_accepts_qv_paged_and_split(built_lib):
    p = _mla()
    assert built_lib.fa_fwd_validate(ctypes.byref(p)) == 0
    assert built_lib.fa_fwd_workspace_size(ctypes.byref(p)) == 0
    p = _mla()
    p.block_table, p.block_table_batch_stride, p.page_block_size = 0x200000, 64, 64
    for t in ("k", "v"):
        setattr(p, f"{t}_batch_stride", 64 * (64 + 512))
    assert built_lib.fa_fwd_validate(ctypes.byref(p)) == 0
    p = _mla()
    p.num_splits = 4
    _with_workspace(built_lib, p)
    assert built_lib.fa_fwd_validate(ctypes.byref(p)) == 0
    # seqused / leftpad / kv_batch_idx / masks / softcap / chunk are all accepted with qv
    p = _mla(sq=4)
    p.seqused_k, p.leftpad_k, p.kv_batch_idx = 0x300000, 0x300100, 0x300200
    p.is_causal, p.softcap, p.attention_chunk = 1, 30.0, 256
    assert built_lib.fa_fwd_validate(ctypes.byref(p)) == 0
    # without qv: d 64 / d_v 512 on a paged cache and with split-KV (rejected before ABI v13)
    p = _mla()
    p.qv = None
    p.num_splits = 3
    _with_workspace(built_lib, p)
    assert built_lib.fa_fwd_validate(ctypes.byref(p)) == 0
    p = _mla()
    p.qv = None
    p.block_table, p.block_table_batch_stride, p.page_block_size = 0x200000, 64, 16
    assert built_lib.fa_fwd_validate(ctypes.byref(p)) == 0


@pytest.mark.parametrize("mutate,code", [
    (lambda p: setattr(p, "d", 128), -7),                       # q/k head dim > 64
    (lambda p: setattr(p, "d_v", 128), -7),                     # V head dim < 256
    (lambda p: setattr(p, "dtype", _lib.FA_DTYPE_FP8_E4M3), -7),  # no fp8 qv
    (lambda p: setattr(p, "alibi_slopes", 0x400000), -7),  # FA3 has no ALiBi
    (lambda p: setattr(p, "d_v", 520), -3),                     # the head-dim rule keeps its code
    (lambda p: setattr(p, "qv_row_stride", 4), -6),             # qv rows 16-byte aligned
    (lambda p: setattr(p, "qv", 0x100008), -6),
])
def test_validate_rejects_qv(built_lib, mutate, code):
    p = _mla()
    mutate(p)
    assert built_lib.fa_fwd_validate(ctypes.byref(p)) == code


def test_qv_dropout_rejected(built_lib):
    p = _mla()
    p.p_dropout, p.rng_state = 0.1, 0x500000
    assert built_lib.fa_fwd_validate(ctypes.byref(p)) == -7


def test_split_qv_workspace_formula(built_lib):
    """fp32 partial O (splits, b, sq, h, d_v) + LSE (splits, b, h, sq), each rounded up to 256 bytes."""
    rnd = lambda x: (x + 255) // 256 * 256  # noqa: E731
    for b, sq, h, dv, splits in ((4, 1, 16, 512, 4), (3, 2, 128, 384, 3), (1, 4, 8, 256, 7)):
        p = _mla(b=b, sq=sq, h=h, dv=dv)
        p.num_splits = splits
        want = rnd(splits * b * sq * h * dv * 4) + rnd(splits * b * h * sq * 4)
        assert built_lib.fa_fwd_workspace_size(ctypes.byref(p)) == want
        p.workspace, p.workspace_bytes = 0x10000000, want - 256
        assert built_lib.fa_fwd_validate(ctypes.byref(p)) == -11
    # heuristic: MLA decode with few (batch, kv head) groups splits the key range, deterministically
    p = _mla(b=1, sk=8192)
    p.num_splits = 0
    n1 = built_lib.fa_fwd_workspace_size(ctypes.byref(p))
    assert n1 > 0 and n1 == built_lib.fa_fwd_workspace_size(ctypes.byref(p))


def test_existing_dv_rules_keep_their_codes(built_lib):
    """d_v of its own outside the qv shape: split-KV and paged stay rejected (-7), as before ABI v13."""
    p = _mla(d=64, dv=128)
    p.qv = None
    p.num_splits = 4
    assert built_lib.fa_fwd_validate(ctypes.byref(p)) == -7
    p = _mla(d=128, dv=512)
    p.qv = None
    p.block_table, p.block_table_batch_stride, p.page_block_size = 0x200000, 64, 64
    assert built_lib.fa_fwd_validate(ctypes.byref(p)) == -7


def test_append_d_v_validation(built_lib):
    p = _lib.FaKvcacheAppendParams()
    p.abi_version, p.struct_size = _lib.FA_ABI_VERSION, ctypes.sizeof(p)
    p.b, p.seqlen_new, p.seqlen_cache, p.h_k, p.d, p.d_v = 1, 0, 16, 1, 64, 520
    assert built_lib.fa_kvcache_append(ctypes.byref(p), None) == -3
    p.d_v = 512
    assert built_lib.fa_kvcache_append(ctypes.byref(p), None) == 0  # (seqlen_new 0: nothing to do, no launch)


def test_qv_kernel_isa_no_scratch(tmp_path):
    """The qv kernel is in the gfx950 build of fa_fwd_api.hip, in every (dtype, V tile, softcap) form, without scratch."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_hazards
    out = tmp_path / "fa.s"
    csrc = os.path.join(ROOT, "flash_attention_annotated_amd", "csrc")
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                    "-I", csrc, "-S", "--cuda-device-only", os.path.join(csrc, "fa_fwd_api.hip"), "-o", str(out)],
                   check=True, stderr=subprocess.DEVNULL)
    assert not isa_hazards.scan(str(out))
    txt = open(out).read()
    kernels = {m.group(1): m.group(2) for m in
               re.finditer(r"^(_ZN2fa13fwd_kernel_qv\w+):.*?\n(.*?)\.end_amdhsa_kernel", txt, re.S | re.M)}
    assert len(kernels) == 8, sorted(kernels)
    for name, body in kernels.items():
        assert "scratch_" not in body, name
        assert "ds_read_b64_tr_b16" in body and "ds_read_b128" in body and "v_mfma_f32_32x32x16" in body, name
        m = re.search(r"\.set %s\.private_seg_size, (\d+)" % re.escape(name), txt)
        assert m and int(m.group(1)) == 0, name
