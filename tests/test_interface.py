"""CPU tests of the Python host layer: it mirrors the reference's operator interface (names, argument order,
defaults) and it never computes attention on a fallback path."""
import inspect
import os

import pytest
import torch

import flash_attention_annotated_amd as fa
from flash_attention_annotated_amd import bert_padding, flash_attn_2_cuda, sharding


def _params(f):
    return [(n, p.default) for n, p in inspect.signature(f).parameters.items()]


def test_flash_attn_func_signature():
    """flash_attn/flash_attn_interface.py:1145-1157"""
    assert _params(fa.flash_attn_func) == [
        ("q", inspect._empty), ("k", inspect._empty), ("v", inspect._empty), ("dropout_p", 0.0),
        ("softmax_scale", None), ("causal", False), ("window_size", (-1, -1)), ("softcap", 0.0),
        ("alibi_slopes", None), ("deterministic", False), ("return_attn_probs", False)]


def test_flash_attn_varlen_func_signature():
    """flash_attn/flash_attn_interface.py:1380-1397"""
    assert _params(fa.flash_attn_varlen_func) == [
        ("q", inspect._empty), ("k", inspect._empty), ("v", inspect._empty), ("cu_seqlens_q", inspect._empty),
        ("cu_seqlens_k", inspect._empty), ("max_seqlen_q", inspect._empty), ("max_seqlen_k", inspect._empty),
        ("dropout_p", 0.0), ("softmax_scale", None), ("causal", False), ("window_size", (-1, -1)), ("softcap", 0.0),
        ("alibi_slopes", None), ("deterministic", False), ("return_attn_probs", False), ("block_table", None)]


def test_extension_module_is_the_compiled_binding():
    """The five entry points flash_attn_interface.py looks up on flash_attn_2_cuda (:91,:168,:269,:369,:1594),
    with the positional arity of the pybind signatures (csrc/flash_attn/flash_api.cpp:350-363, 514-535), are the
    compiled binding's functions themselves."""
    import re

    def arity(fn):  # pybind functions carry their signature in the first docstring line
        try:
            return len(inspect.signature(fn).parameters)
        except ValueError:
            return len(re.findall(r"\barg\d+:", fn.__doc__.splitlines()[0]))
    want = {"fwd": 13, "varlen_fwd": 21, "bwd": 19, "varlen_bwd": 24, "fwd_kvcache": 20}  # :350-363, 514-535, 767-786, 973-997, 1202-1222
    from flash_attention_annotated_amd import flash_attn_2_cuda_C as compiled
    import flash_attn_2_cuda as top_level_alias  # the name the reference imports
    for name, n in want.items():
        assert callable(getattr(flash_attn_2_cuda, name))
        assert arity(getattr(flash_attn_2_cuda, name)) == n, name
        # the reference's flash_attn_gpu is the compiled module's functions, with nothing in between
        assert getattr(top_level_alias, name) is getattr(flash_attn_2_cuda, name) is getattr(compiled, name), name
        assert type(getattr(top_level_alias, name)).__name__ == "builtin_function_or_method", name
    assert flash_attn_2_cuda._fwd_kvcache_impl is compiled._fwd_kvcache_impl
    # the FA3 forward (hopper/flash_api.cpp:672-705, 34 arguments) is the compiled function too
    from flash_attention_annotated_amd import flash_attn_3_cuda
    assert flash_attn_3_cuda.fwd is compiled.fa3_fwd
    assert type(flash_attn_3_cuda.fwd).__name__ == "builtin_function_or_method"
    assert arity(flash_attn_3_cuda.fwd) == 34
    assert [n for n, _ in _params(fa.flash_attn_with_kvcache)] == [
        "q", "k_cache", "v_cache", "k", "v", "rotary_cos", "rotary_sin", "cache_seqlens", "cache_batch_idx",
        "cache_leftpad", "block_table", "softmax_scale", "causal", "window_size", "softcap", "rotary_interleaved",
        "alibi_slopes", "num_splits", "return_softmax_lse"]  # flash_attn/flash_attn_interface.py:1474-1494


def test_no_cpu_fallback():
    """CPU tensors are rejected like the reference's CHECK_DEVICE does; nothing is computed off the GPU."""
    q = torch.randn(1, 16, 2, 64, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="must be on CUDA"):
        fa.flash_attn_func(q, q, q)
    with pytest.raises(RuntimeError, match="only support fp16 and bf16"):
        fa.flash_attn_func(q.float(), q.float(), q.float())
    # each entry point of the extension module, called directly as the reference's flash_attn_gpu does
    lse = torch.zeros(1, 2, 16)
    qv, lse_v, cu = q[0], torch.zeros(2, 16), torch.tensor([0, 16], dtype=torch.int32)
    cache_seqlens = torch.zeros(1, dtype=torch.int32)
    calls = (
        lambda: flash_attn_2_cuda.fwd(q, q, q, None, None, 0.0, 0.125, False, -1, -1, 0.0, False, None),
        lambda: flash_attn_2_cuda.varlen_fwd(qv, qv, qv, None, cu, cu, None, None, None, None, 16, 16, 0.0, 0.125, False,
                                             False, -1, -1, 0.0, False, None),
        lambda: flash_attn_2_cuda.bwd(q, q, q, q, q, lse, None, None, None, None, 0.0, 0.125, False, -1, -1, 0.0, False, None,
                                      None),
        lambda: flash_attn_2_cuda.varlen_bwd(qv, qv, qv, qv, qv, lse_v, None, None, None, cu, cu, None, 16, 16, 0.0, 0.125,
                                             False, False, -1, -1, 0.0, False, None, None),
        lambda: flash_attn_2_cuda.fwd_kvcache(q, q, q, None, None, cache_seqlens, None, None, None, None, None, None, None,
                                              0.125, False, -1, -1, 0.0, False, 0),
    )
    # the compiled FA3 entry points: forward (dense, varlen), backward (d_v == d, d_v != d), combine
    from flash_attention_annotated_amd import _lib, flash_attn_3_cuda
    binding = _lib.binding()

    def fa3_fwd(q, k, v, cu_seqlens=None, max_seqlen=None):
        return flash_attn_3_cuda.fwd(q, k, v, None, None, None, None, cu_seqlens, cu_seqlens, None, None, None, max_seqlen,
                                     max_seqlen, None, None, None, None, None, None, None, None, None, None, False, -1, -1, 0,
                                     0.0, False, None, 1, None, 0)

    def fa3_bwd(q, k, v, out, lse, cu_seqlens=None, max_seqlen=None):
        return binding.fa3_bwd(out, q, k, v, out, lse, None, None, None, cu_seqlens, cu_seqlens, None, None, max_seqlen,
                               max_seqlen, None, False, -1, -1, 0.0, False, 0)
    q192, v128 = torch.randn(1, 16, 2, 192, dtype=torch.bfloat16), torch.randn(1, 16, 2, 128, dtype=torch.bfloat16)
    calls += (
        lambda: fa3_fwd(q, q, q),
        lambda: fa3_fwd(qv, qv, qv, cu, 16),
        lambda: fa3_bwd(q, q, q, q, lse),
        lambda: fa3_bwd(q192, q192, v128, v128, lse),
        lambda: binding.fa3_fwd_combine(torch.randn(2, 1, 16, 2, 64), torch.randn(2, 1, 16, 2), None, None),
    )
    for call in calls:
        with pytest.raises(RuntimeError, match="must be on CUDA"):
            call()
    with pytest.raises(RuntimeError, match="FlashAttention only supports fp16, bf16, and fp8_e4m3 data type"):
        fa3_fwd(q.float(), q.float(), q.float())


def test_package_import_does_not_load_the_binding():
    """The compiled binding is resolved on first use, so the package imports before build() has run (test collection
    imports it before conftest.py builds)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = (f"import sys; sys.path.insert(0, {root!r}); import flash_attention_annotated_amd; "
            "import flash_attention_annotated_amd.hopper_interface; "
            "assert 'flash_attention_annotated_amd.flash_attn_2_cuda_C' not in sys.modules")
    subprocess.run([sys.executable, "-c", code], check=True)


def test_fa_fwd_lib_override_reaches_the_binding(tmp_path):
    """FA_FWD_LIB (developer override: ablation / instrumented builds) names the library instance that every compiled call
    resolves to.  In a child process: conftest.py refuses the variable in the test session itself."""
    import shutil
    import subprocess
    import sys
    from flash_attention_annotated_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    copy = str(tmp_path / "libfa_override.so")
    shutil.copyfile(_lib.LIB_PATH, copy)
    code = (f"import sys, ctypes; sys.path.insert(0, {root!r})\n"
            "from flash_attention_annotated_amd import flash_attn_2_cuda\n"
            "flash_attn_2_cuda.fwd\n"
            "class DlInfo(ctypes.Structure):\n"
            "    _fields_ = [('dli_fname', ctypes.c_char_p), ('dli_fbase', ctypes.c_void_p), ('dli_sname', ctypes.c_char_p),\n"
            "                ('dli_saddr', ctypes.c_void_p)]\n"
            "libdl = ctypes.CDLL(None)\n"
            "libdl.dlsym.restype = ctypes.c_void_p\n"
            "libdl.dlsym.argtypes = [ctypes.c_void_p, ctypes.c_char_p]\n"
            "libdl.dladdr.argtypes = [ctypes.c_void_p, ctypes.POINTER(DlInfo)]\n"
            "addr = libdl.dlsym(None, b'fa_fwd')  # RTLD_DEFAULT\n"
            "info = DlInfo()\n"
            "assert addr and libdl.dladdr(addr, ctypes.byref(info)), 'fa_fwd is not resolvable'\n"
            "print(info.dli_fname.decode())\n")
    env = dict(os.environ, FA_FWD_LIB=copy)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert os.path.realpath(r.stdout.strip().splitlines()[-1]) == os.path.realpath(copy), r.stdout


def test_unpad_pad_roundtrip():
    torch.manual_seed(0)
    x = torch.randn(3, 7, 2, 4)
    mask = torch.tensor([[1, 1, 1, 0, 0, 0, 0], [1, 1, 1, 1, 1, 1, 1], [1, 0, 0, 0, 0, 0, 0]], dtype=torch.bool)
    xu, idx, cu, mx, used = bert_padding.unpad_input(x, mask)
    assert cu.tolist() == [0, 3, 10, 11] and cu.dtype == torch.int32 and mx == 7 and used.tolist() == [3, 7, 1]
    back = bert_padding.pad_input(xu, idx, 3, 7)
    assert torch.equal(back[mask], x[mask]) and torch.all(back[~mask] == 0)


def test_shard_range_partitions():
    for n in (1, 4, 7, 32):
        for world in (1, 2, 3, 8):
            spans = [sharding.shard_range(n, r, world) for r in range(world)]
            assert spans[0][0] == 0 and spans[-1][1] == n
            assert all(spans[i][1] == spans[i + 1][0] for i in range(world - 1))
            sizes = [b - a for a, b in spans]
            assert max(sizes) - min(sizes) <= 1


def test_torch_library_ops_have_fake_implementations():
    """torch.compile surface (reference flash_attn/flash_attn_interface.py:76,109-136,241,292-325): the host entry
    points are custom ops whose fake kernels give the shapes of the real ones; meta tensors exercise them."""
    q = torch.empty(2, 100, 4, 64, dtype=torch.bfloat16, device="meta")
    k = torch.empty(2, 130, 2, 64, dtype=torch.bfloat16, device="meta")
    out, lse, p, rng = torch.ops.flash_attn_amd._flash_attn_forward(q, k, k, 0.0, 0.125, True, -1, -1, 0.0, None, False)
    assert out.shape == q.shape and lse.shape == (2, 4, 100) and lse.dtype == torch.float32 and p.shape == (0,)
    sd = torch.ops.flash_attn_amd._flash_attn_backward(out, q, k, k, out, lse, torch.empty_like(q), torch.empty_like(k),
                                                       torch.empty_like(k), 0.0, 0.125, True, -1, -1, 0.0, None, False)
    assert sd.shape == (2, 4, 128)
    qv = torch.empty(393, 4, 64, dtype=torch.float16, device="meta")
    cu = torch.empty(4, dtype=torch.int32, device="meta")
    out, lse, _, _ = torch.ops.flash_attn_amd._flash_attn_varlen_forward(qv, qv, qv, cu, cu, 256, 256, 0.0, 0.125, False)
    assert out.shape == qv.shape and lse.shape == (4, 393)
    sd = torch.ops.flash_attn_amd._flash_attn_varlen_backward(out, qv, qv, qv, out, lse, None, None, None, cu, cu, 256,
                                                              256, 0.0, 0.125, False, -1, -1, 0.0, None, False)
    assert sd.shape == (4, 393 + 128 * 3)


def test_attention_modules_mirror_the_reference_constructors():
    from flash_attention_annotated_amd.modules.mha import FlashCrossAttention, FlashSelfAttention
    sa = FlashSelfAttention(causal=True, softmax_scale=0.1, attention_dropout=0.0, window_size=(4, 0))
    ca = FlashCrossAttention(causal=False, alibi_slopes=torch.rand(4))
    assert [p for p in inspect.signature(sa.forward).parameters] == ["qkv", "causal", "cu_seqlens", "max_seqlen"]
    assert [p for p in inspect.signature(ca.forward).parameters] == [
        "q", "kv", "causal", "cu_seqlens", "max_seqlen", "cu_seqlens_k", "max_seqlen_k"]
    with pytest.raises(AssertionError):
        sa(torch.randn(1, 8, 3, 2, 64, dtype=torch.bfloat16))  # CPU tensor: rejected like the reference does


def test_flash3_bw_compatibility():
    """hopper/test_flash_attn.py:1163-1201: the four `flash_attn_3` op schemas stay backward compatible with the
    reference's (arguments only appended with defaults).  The strings below are the reference test's."""
    from torch._C import parse_schema
    import flash_attention_annotated_amd.hopper_interface  # noqa: F401  (registers torch.ops.flash_attn_3)
    assert torch.ops.flash_attn_3.fwd.default._schema.is_backward_compatible_with(parse_schema(
        "flash_attn_3::fwd(Tensor q, Tensor k, Tensor v, Tensor(k_new!)? k_new=None, "
        "Tensor(v_new!)? v_new=None, Tensor? q_v=None, Tensor(out!)? out=None, "
        "Tensor? cu_seqlens_q=None, Tensor? cu_seqlens_k=None, "
        "Tensor? cu_seqlens_k_new=None, Tensor? seqused_q=None, Tensor? seqused_k=None, "
        "int? max_seqlen_q=None, int? max_seqlen_k=None, Tensor? page_table=None, "
        "Tensor? kv_batch_idx=None, Tensor? leftpad_k=None, Tensor? rotary_cos=None, Tensor? rotary_sin=None, "
        "Tensor? seqlens_rotary=None, Tensor? q_descale=None, Tensor? k_descale=None, Tensor? v_descale=None, "
        "float? softmax_scale=None, bool is_causal=False, int window_size_left=-1, int window_size_right=-1, "
        "int attention_chunk=0, float softcap=0., bool is_rotary_interleaved=False, "
        "Tensor? scheduler_metadata=None, int num_splits=0, bool? pack_gqa=None, int sm_margin=0) "
        "-> (Tensor(out!), Tensor, Tensor, Tensor)"))
    assert torch.ops.flash_attn_3.bwd.default._schema.is_backward_compatible_with(parse_schema(
        "flash_attn_3::bwd(Tensor dout, Tensor q, Tensor k, Tensor v, Tensor out, Tensor softmax_lse, "
        "Tensor(dq!)? dq=None, Tensor(dk!)? dk=None, Tensor(dv!)? dv=None, Tensor? cu_seqlens_q=None, "
        "Tensor? cu_seqlens_k=None, Tensor? seqused_q=None, Tensor? seqused_k=None, int? max_seqlen_q=None, "
        "int? max_seqlen_k=None, float? softmax_scale=None, bool is_causal=False, int window_size_left=-1, "
        "int window_size_right=-1, float softcap=0., bool deterministic=False, int sm_margin=0) "
        "-> (Tensor(dq!), Tensor(dk!), Tensor(dv!), Tensor, Tensor, Tensor, Tensor, Tensor)"))
    assert torch.ops.flash_attn_3.fwd_combine.default._schema.is_backward_compatible_with(parse_schema(
        "flash_attn_3::fwd_combine(Tensor out_partial, Tensor lse_partial, Tensor(out!)? out=None, "
        "ScalarType? out_dtype=None) -> (Tensor(out!), Tensor)"))
    assert torch.ops.flash_attn_3.get_scheduler_metadata.default._schema.is_backward_compatible_with(parse_schema(
        "flash_attn_3::get_scheduler_metadata(int batch_size, int max_seqlen_q, int max_seqlen_k, "
        "int num_heads, int num_heads_k, int headdim, int headdim_v, ScalarType qkv_dtype, Tensor seqused_k, "
        "Tensor? cu_seqlens_q=None, Tensor? cu_seqlens_k=None, Tensor? cu_seqlens_k_new=None, "
        "Tensor? seqused_q=None, Tensor? leftpad_k=None, int? page_size=None, int max_seqlen_k_new=0, "
        "bool is_causal=False, int window_size_left=-1, int window_size_right=-1, "
        "int attention_chunk=0, bool has_softcap=False, int num_splits=0, bool? pack_gqa=None, "
        "int sm_margin=0) -> Tensor"))
