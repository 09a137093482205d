"""GPU parity tests of the HIP forward against the oracle, through the public API and the C-ABI.

Ports the reference's tolerance contract as inequalities:
  FA2  |out - out_ref|max <= 2 * |out_pt - out_ref|max (+1e-5 in the causal tests)
       tests/test_flash_attn.py:1121,1440,1556
  FA3  <= rtol * |out_pt - out_ref|max + fwd_atol, fwd_atol = 2*|(out_ref + 0.3 - 0.3) - out_ref|max
       hopper/test_flash_attn.py:193-194,223
The bound used here is the FA2 one plus the FA3 atol (floating point; tolerance stated per test).
"""
import math

import pytest
import torch

from oracle import attention_ref as oracle
from oracle.cases import CASES, checksum, make_alibi_slopes, make_inputs, padding_masks
from parity_helpers import last_plan

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _api():
    import flash_attention_annotated_amd as fa
    return fa


def _bound(out_ref, out_pt):
    fwd_atol = 2 * (out_ref + 0.3 - 0.3 - out_ref).abs().max().item()
    return 2 * (out_pt.float() - out_ref.float()).abs().max().item() + fwd_atol + 1e-5


def _check(out, out_ref, out_pt, what=""):
    err = (out.float().cpu() - out_ref.float()).abs().max().item()
    bound = _bound(out_ref.float(), out_pt)
    assert math.isfinite(err), f"{what}: non-finite output"
    assert err <= bound, f"{what}: max err {err:.3e} > bound {bound:.3e}"
    return err, bound


def _dense_ref(q, k, v, **kw):
    out_ref, _, lse = oracle.attention_ref(q, k, v, **kw, return_lse=True)
    out_pt, _ = oracle.attention_ref(q, k, v, **kw, upcast=False, reorder_ops=True)
    return out_ref, out_pt, lse


def _check_lse(lse, lse_ref, tol=2e-3):
    lse = lse.float().cpu()
    fin = torch.isfinite(lse_ref)
    assert torch.equal(torch.isfinite(lse), fin), "lse inf pattern differs"
    assert torch.equal(lse[~fin], lse_ref[~fin]), "lse +inf rows differ"
    if fin.any():
        err = (lse[fin] - lse_ref[fin]).abs().max().item()
        assert err <= tol, f"lse err {err:.3e}"


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c["dtype"] != "fp32" and not c.get("fp8")])
def test_golden_cases(name, golden):
    """Every 16-bit golden case: HIP output vs the reference's frozen out_ref / out_pt."""
    fa = _api()
    c = CASES[name]
    g = golden[name]
    q, k, v = make_inputs(c)
    assert abs(checksum(q) - g["input_checksum"][0].item()) < 1e-6
    qm, km = padding_masks(c)
    stride = c["store_row_stride"]
    kw = dict(causal=c["causal"], window_size=c["window"], softcap=c["softcap"])
    slopes = make_alibi_slopes(c)
    lse_ref = g["lse"]
    if slopes is not None:
        kw["alibi_slopes"] = slopes.to(DEV)
        # the kernel's LSE carries the general bias -slope*|i + sk - sq - j| (include/fa_fwd.h); the frozen causal
        # fixture was made with the reference's causal shortcut slope*(j - sk + 1), a per-row constant apart
        bias = oracle.attn_bias_from_alibi_slopes(slopes, c["sq"], c["sk"], qm, km, causal=False)
        lse_ref = oracle.attention_ref(q, k, v, qm, km, attn_bias=bias, causal=c["causal"], window_size=c["window"],
                                       softcap=c["softcap"], return_lse=True)[2][:, :, ::stride]
    if qm is None:
        out, lse, _ = fa.flash_attn_func(q.to(DEV), k.to(DEV), v.to(DEV), **kw, return_attn_probs=True)
    else:
        from flash_attention_annotated_amd.bert_padding import pad_input, unpad_input
        qu, iq, cuq, mq, _ = unpad_input(q, qm)
        ku, ik, cuk, mk, _ = unpad_input(k, km)
        vu = unpad_input(v, km)[0]
        out_u = fa.flash_attn_varlen_func(qu.to(DEV), ku.to(DEV), vu.to(DEV), cuq.to(DEV), cuk.to(DEV), mq, mk, **kw)
        out = pad_input(out_u.cpu(), iq, c["b"], c["sq"])
        lse = None
    err, bound = _check(out[:, ::stride], g["out_ref_fp32"], g["out_pt"], name)
    if lse is not None:
        _check_lse(lse[:, :, ::stride], lse_ref)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("sq,sk,d", [(113, 203, 64), (512, 512, 128), (1024, 1023, 64), (203, 113, 256), (2048, 2048, 128),
                                     (1500, 1500, 40), (1300, 1700, 96), (1024, 2048, 160), (1111, 1111, 192), (1536, 1536, 256)])
@pytest.mark.parametrize("per_batch", [False, True])
def test_alibi(sq, sk, d, causal, per_batch):
    """ALiBi slopes (h) or (b, h), rand * 0.3 as tests/test_flash_attn.py:936-940; oracle bias from
    attn_bias_from_alibi_slopes (:29-56, restated in oracle/ and pinned to the reference by make_golden.py).  The long sweeps
    run the ALIBI form of the generated loop (FastLoop256<T, DEFF, false, true>: the 32-row-per-wave kernel shape at every head
    dim, chosen by plan_fwd in fa_fwd_api.hip below 129), entered and left at the causal diagonal and the sequence tail."""
    fa = _api()
    torch.manual_seed(11)
    b, h, hk = 2, 4, 2
    q = torch.randn(b, sq, h, d, dtype=torch.bfloat16)
    k = torch.randn(b, sk, hk, d, dtype=torch.bfloat16)
    v = torch.randn(b, sk, hk, d, dtype=torch.bfloat16)
    slopes = torch.rand(b, h, dtype=torch.float32) * 0.3
    if not per_batch:
        slopes = slopes[:1].expand(b, h).contiguous()
    arg = slopes if per_batch else slopes[0].contiguous()
    out, lse, _ = fa.flash_attn_func(q.to(DEV), k.to(DEV), v.to(DEV), causal=causal, alibi_slopes=arg.to(DEV),
                                     return_attn_probs=True)
    bias = oracle.attn_bias_from_alibi_slopes(slopes, sq, sk, causal=False)
    out_ref, out_pt, lse_ref = _dense_ref(q, k, v, causal=causal, attn_bias=bias)
    _check(out, out_ref, out_pt, f"alibi {sq}x{sk} d{d} causal={causal}")
    _check_lse(lse, lse_ref)
    if causal:  # the reference's causal shortcut bias gives the same output
        bias_c = oracle.attn_bias_from_alibi_slopes(slopes, sq, sk, causal=True)
        out_ref_c, out_pt_c, _ = _dense_ref(q, k, v, causal=True, attn_bias=bias_c)
        _check(out, out_ref_c, out_pt_c, "alibi causal shortcut")


def test_alibi_varlen_softcap():
    """ALiBi through the varlen entry point (per-sequence sk - sq shift) together with softcap."""
    fa = _api()
    from flash_attention_annotated_amd.bert_padding import pad_input, unpad_input
    torch.manual_seed(12)
    b, sq, sk, h, d = 3, 150, 190, 4, 64
    q = torch.randn(b, sq, h, d, dtype=torch.float16) * 4
    k = torch.randn(b, sk, h, d, dtype=torch.float16)
    v = torch.randn(b, sk, h, d, dtype=torch.float16)
    qm = torch.arange(sq).view(1, -1) < torch.tensor([[150], [131], [140]])
    km = torch.arange(sk).view(1, -1) < torch.tensor([[171], [190], [175]])
    slopes = torch.rand(b, h, dtype=torch.float32) * 0.3
    qu, iq, cuq, mq, _ = unpad_input(q, qm)
    ku, ik, cuk, mk, _ = unpad_input(k, km)
    vu = unpad_input(v, km)[0]
    out_u = fa.flash_attn_varlen_func(qu.to(DEV), ku.to(DEV), vu.to(DEV), cuq.to(DEV), cuk.to(DEV), mq, mk,
                                      softcap=20.0, alibi_slopes=slopes.to(DEV))
    out = pad_input(out_u.cpu(), iq, b, sq)
    bias = oracle.attn_bias_from_alibi_slopes(slopes, sq, sk, qm, km)
    out_ref, _ = oracle.attention_ref(q, k, v, qm, km, attn_bias=bias, softcap=20.0)
    out_pt, _ = oracle.attention_ref(q, k, v, qm, km, attn_bias=bias, softcap=20.0, upcast=False, reorder_ops=True)
    _check(out, out_ref, out_pt, "alibi varlen softcap")


SHAPES = [(1, 1), (1, 147), (64, 128), (113, 203), (128, 217), (203, 113), (256, 256), (257, 1), (384, 256),
          (512, 512), (1023, 1024), (1024, 1023), (2048, 2048)]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("sq,sk", SHAPES)
@pytest.mark.parametrize("mha_type", ["mha", "gqa", "mqa"])
def test_dense_output(sq, sk, d, causal, dtype, mha_type):
    """Shape matrix in the style of tests/test_flash_attn.py:878-919 (batch 4 -> 2, heads 6)."""
    if mha_type != "mha" and (sq, sk) not in [(113, 203), (512, 512), (1023, 1024)]:
        pytest.skip("gqa/mqa on a subset of shapes")
    if dtype == torch.float16 and sq >= 2048:
        pytest.skip("fp16 on the CPU oracle is slow at this size (7-14 s per case); covered in bf16")
    fa = _api()
    torch.manual_seed(0)
    b, h = 2, 6
    hk = {"mha": 6, "gqa": 2, "mqa": 1}[mha_type]
    q = torch.randn(b, sq, h, d, dtype=dtype)
    k = torch.randn(b, sk, hk, d, dtype=dtype)
    v = torch.randn(b, sk, hk, d, dtype=dtype)
    out, lse, _ = fa.flash_attn_func(q.to(DEV), k.to(DEV), v.to(DEV), causal=causal, return_attn_probs=True)
    out_ref, out_pt, lse_ref = _dense_ref(q, k, v, causal=causal)
    _check(out, out_ref, out_pt, f"{sq}x{sk} d{d} causal={causal} {mha_type}")
    _check_lse(lse, lse_ref)


@pytest.mark.parametrize("d", [32, 40, 59, 96, 111, 160, 192, 224, 256])
@pytest.mark.parametrize("causal", [False, True])
def test_head_dims(d, causal):
    """Head dims of tests/test_flash_attn.py:878 that are not a tile width: padded to x8 by the Python
    layer (flash_attn_interface.py:839-843) and to the tile width inside the kernel."""
    fa = _api()
    torch.manual_seed(1)
    q = torch.randn(2, 217, 4, d, dtype=torch.bfloat16)
    k = torch.randn(2, 330, 2, d, dtype=torch.bfloat16)
    v = torch.randn(2, 330, 2, d, dtype=torch.bfloat16)
    out = fa.flash_attn_func(q.to(DEV), k.to(DEV), v.to(DEV), causal=causal)
    assert out.shape == q.shape
    out_ref, out_pt, _ = _dense_ref(q, k, v, causal=causal)
    _check(out, out_ref, out_pt, f"d={d}")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("d", [160, 192, 256])
@pytest.mark.parametrize("sq,sk,causal,window", [(1024, 1024, False, (-1, -1)), (1024, 1024, True, (-1, -1)),
                                                 (777, 1301, True, (-1, -1)), (1301, 777, False, (-1, -1)),
                                                 (1024, 1536, False, (300, 0)), (900, 1100, False, (257, 130))])
def test_head_dim_tile_256(sq, sk, causal, window, d, dtype):
    """Head dims 129 .. 256 on their own kernel (fa_fwd_kernel_d256.h: 4 waves x 32 rows around the generated loop FastLoop256):
    sweeps long enough that the generated block runs many tiles, entered and left at masks (causal diagonal, window edges,
    sequence tails), GQA 4/2, both 16-bit types; LSE included."""
    fa = _api()
    torch.manual_seed(sq + sk + d)
    q = torch.randn(2, sq, 4, d, dtype=dtype)
    k = torch.randn(2, sk, 2, d, dtype=dtype)
    v = torch.randn(2, sk, 2, d, dtype=dtype)
    out, lse, _ = fa.flash_attn_func(q.to(DEV), k.to(DEV), v.to(DEV), causal=causal, window_size=window, return_attn_probs=True)
    ref_window = (window[0], sk) if (window[0] >= 0 and window[1] < 0) else window
    out_ref, out_pt, lse_ref = _dense_ref(q, k, v, causal=causal, window_size=ref_window)
    _check(out, out_ref, out_pt, f"d={d} {sq}x{sk} causal={causal} window={window}")
    _check_lse(lse, lse_ref)


def test_head_dim_tile_256_varlen_and_forced_trip():
    """The d256 kernel on a ragged batch (cu_seqlens, lengths 1 .. 900), and its guard: a key that dominates one row late in
    the sweep makes the partial row sums of the generated block overflow the stale max (the block is left, P redone from the
    kept scores with a fresh max, O rescaled)."""
    fa = _api()
    torch.manual_seed(77)
    d, h, hk = 192, 4, 2
    lens = [900, 1, 333, 64, 517]
    cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32)
    tot = int(cu[-1])
    q = torch.randn(tot, h, d, dtype=torch.bfloat16)
    k = torch.randn(tot, hk, d, dtype=torch.bfloat16)
    v = torch.randn(tot, hk, d, dtype=torch.bfloat16)
    out = fa.flash_attn_varlen_func(q.to(DEV), k.to(DEV), v.to(DEV), cu.to(DEV), cu.to(DEV), max(lens), max(lens), causal=True)
    ref, _ = oracle.attention_varlen_ref(q, k, v, cu, cu, causal=True)
    pt, _ = oracle.attention_varlen_ref(q, k, v, cu, cu, causal=True, upcast=False, reorder_ops=True)
    _check(out, ref, pt, "d192 varlen causal")
    # forced trip: rows 40 (wave 1) and 300 meet their dominant key in tiles 9 and 14 of a 1024-key sweep
    sq, sk, d = 512, 1024, 256
    q = torch.randn(1, sq, 2, d, dtype=torch.bfloat16)
    k = torch.randn(1, sk, 2, d, dtype=torch.bfloat16)
    v = torch.randn(1, sk, 2, d, dtype=torch.bfloat16)
    k[0, 600, 0] = q[0, 40, 0] * 3.0
    k[0, 950, 1] = q[0, 300, 1] * 3.0
    out, lse, _ = fa.flash_attn_func(q.to(DEV), k.to(DEV), v.to(DEV), return_attn_probs=True)
    out_ref, out_pt, lse_ref = _dense_ref(q, k, v)
    _check(out, out_ref, out_pt, "d256 forced guard trip")
    _check_lse(lse, lse_ref, tol=5e-3)


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("window", [(300, 0), (256, 100), (700, -1), (130, 64)])
@pytest.mark.parametrize("sq,sk", [(1536, 1536), (1200, 1700)])
def test_sliding_window_long(sq, sk, window, d):
    """Windows much shorter than the sequence: behind the left edge of a wave's key range the generated loop takes over (the
    tiles between the two window edges need no mask), the MASKED block does the diagonal; the left-edge tiles stay generic."""
    fa = _api()
    torch.manual_seed(5)
    q = torch.randn(1, sq, 2, d, dtype=torch.bfloat16)
    k = torch.randn(1, sk, 2, d, dtype=torch.bfloat16)
    v = torch.randn(1, sk, 2, d, dtype=torch.bfloat16)
    out, lse, _ = fa.flash_attn_func(q.to(DEV), k.to(DEV), v.to(DEV), window_size=window, return_attn_probs=True)
    ref_window = (window[0], sk) if (window[0] >= 0 and window[1] < 0) else window
    out_ref, out_pt, lse_ref = _dense_ref(q, k, v, window_size=ref_window)
    _check(out, out_ref, out_pt, f"window={window} d={d}")
    _check_lse(lse, lse_ref)


@pytest.mark.parametrize("sq,sk,window", [(448, 704, (96, 64)), (640, 640, (130, 0)), (512, 768, (200, 40))])
def test_sliding_window_seeds(sq, sk, window):
    """Twelve data sets per shape (GQA 4/2, head dim 128; small enough to run split-KV, so key ranges end inside the window):
    regression test of the phantom half-step that trips guard A -- before the fix 2 of the first shape's
    (seed, head) cases came out with LSE + 0.2 on one q-block."""
    fa = _api()
    for seed in range(12):
        torch.manual_seed(seed)
        q = torch.randn(1, sq, 4, 128, dtype=torch.bfloat16)
        k = torch.randn(1, sk, 2, 128, dtype=torch.bfloat16)
        v = torch.randn(1, sk, 2, 128, dtype=torch.bfloat16)
        out, lse, _ = fa.flash_attn_func(q.to(DEV), k.to(DEV), v.to(DEV), window_size=window, return_attn_probs=True)
        out_ref, out_pt, lse_ref = _dense_ref(q, k, v, window_size=window)
        _check(out, out_ref, out_pt, f"window={window} seed={seed}")
        _check_lse(lse, lse_ref)


@pytest.mark.parametrize("window", [(64, 0), (16, 16), (0, 32), (300, -1), (-1, 17), (0, 0)])
@pytest.mark.parametrize("sq,sk", [(113, 203), (512, 512), (700, 333)])
def test_local_window(sq, sk, window):
    fa = _api()
    torch.manual_seed(2)
    q = torch.randn(2, sq, 4, 64, dtype=torch.bfloat16)
    k = torch.randn(2, sk, 2, 64, dtype=torch.bfloat16)
    v = torch.randn(2, sk, 2, 64, dtype=torch.bfloat16)
    out, lse, _ = fa.flash_attn_func(q.to(DEV), k.to(DEV), v.to(DEV), window_size=window, return_attn_probs=True)
    # One-sided windows: the reference's kernel path sets the other side to seqlen_k
    # (set_params_fprop, csrc/flash_attn/flash_api.cpp:141-142) while its test-util mask builder takes a -1 right
    # window literally when left >= 0 (tests/test_util.py:176-182; the reference's own tests never pass that
    # combination).  The kernel-path semantics are the contract: give the oracle the same two-sided window.
    ref_window = (window[0], sk) if (window[0] >= 0 and window[1] < 0) else window
    out_ref, out_pt, lse_ref = _dense_ref(q, k, v, window_size=ref_window)
    _check(out, out_ref, out_pt, f"window={window}")
    _check_lse(lse, lse_ref)


@pytest.mark.parametrize("causal", [False, True])
def test_softcap(causal):
    fa = _api()
    torch.manual_seed(3)
    softcap = 30.0
    q = torch.randn(2, 300, 4, 128, dtype=torch.bfloat16) * (softcap / 4)
    k = torch.randn(2, 421, 4, 128, dtype=torch.bfloat16)
    v = torch.randn(2, 421, 4, 128, dtype=torch.bfloat16)
    out = fa.flash_attn_func(q.to(DEV), k.to(DEV), v.to(DEV), causal=causal, softcap=softcap)
    out_ref, out_pt, _ = _dense_ref(q, k, v, causal=causal, softcap=softcap)
    err = (out.float().cpu() - out_ref.float()).abs().max().item()
    # rtol 3 with softcap, hopper/test_flash_attn.py:194
    bound = 3 * (out_pt.float() - out_ref.float()).abs().max().item() + 2 * (out_ref + 0.3 - 0.3 - out_ref).abs().max().item()
    assert err <= bound, (err, bound)


@pytest.mark.parametrize("d,dtype", [(40, torch.bfloat16), (64, torch.bfloat16), (72, torch.float16), (96, torch.bfloat16), (128, torch.bfloat16),
                                     (128, torch.float16), (160, torch.bfloat16), (192, torch.float16), (256, torch.bfloat16), (256, torch.float16)])
@pytest.mark.parametrize("sq,sk,causal,window", [(1024, 1024, False, (-1, -1)), (777, 1301, True, (-1, -1)),
                                                 (1024, 1536, False, (300, 0)), (400, 400, False, (-1, -1))])
def test_softcap_head_dim_tile_256(sq, sk, causal, window, d, dtype):
    """Softcap on the head-dim-256 tile: the generated block FastLoop256<T, DEFF, true> caps the fresh scores in place (two
    interleaved tanh chains per score pair) and hands already-capped scores to the generic half-step on a guard trip; scores
    pushed into the tanh knee like hopper/test_flash_attn.py:139-140; rtol 3 with softcap (:194).  LSE included.  One case
    per shape also spikes a key late in the sweep so that the guard trips inside a capped block.  Head dims <= 128 with softcap
    take the same kernel shape (DEFF = 64 / 96 / 128 instantiations, chosen by plan_fwd in fa_fwd_api.hip; short causal sweeps at head dim
    <= 64 keep the 4-wave x 32-row compiler-scheduled shape)."""
    fa = _api()
    torch.manual_seed(sq + sk + d)
    softcap = 15.0
    q = torch.randn(2, sq, 4, d, dtype=dtype) * (softcap / 4)
    k = torch.randn(2, sk, 2, d, dtype=dtype)
    v = torch.randn(2, sk, 2, d, dtype=dtype)
    if sk >= 1024:  # after ~12 tiles of scores near -softcap one key reaches +softcap for row 40: partial sums >> 2^THR
        q[0, 40, 0] = q[0, 40, 0].abs()
        k[0, : sk - 200, 0] = -k[0, : sk - 200, 0].abs() * 0.5
        k[0, sk - 150, 0] = k[0, sk - 150, 0].abs() * 2
    out, lse, _ = fa.flash_attn_func(q.to(DEV), k.to(DEV), v.to(DEV), causal=causal, window_size=window, softcap=softcap,
                                     return_attn_probs=True)
    ref_window = (window[0], sk) if (window[0] >= 0 and window[1] < 0) else window
    out_ref, out_pt, lse_ref = _dense_ref(q, k, v, causal=causal, window_size=ref_window, softcap=softcap)
    err = (out.float().cpu() - out_ref.float()).abs().max().item()
    bound = 3 * (out_pt.float() - out_ref.float()).abs().max().item() + 2 * (out_ref + 0.3 - 0.3 - out_ref).abs().max().item()
    assert err <= bound, (err, bound)
    _check_lse(lse, lse_ref, tol=5e-3)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("sq,sk", [(1, 147), (113, 203), (128, 217), (512, 512), (1024, 1024)])
def test_varlen_output(sq, sk, d, causal):
    """Ragged batches with lengths in [max-20, max] (tests/test_flash_attn.py:58-71,1172-1451)."""
    fa = _api()
    from flash_attention_annotated_amd.bert_padding import pad_input, unpad_input
    torch.manual_seed(4)
    b, h, hk = 5, 6, 2
    q = torch.randn(b, sq, h, d, dtype=torch.bfloat16)
    k = torch.randn(b, sk, hk, d, dtype=torch.bfloat16)
    v = torch.randn(b, sk, hk, d, dtype=torch.bfloat16)
    g = torch.Generator().manual_seed(5)
    qm = torch.arange(sq).view(1, -1) < torch.randint(max(1, sq - 20), sq + 1, (b, 1), generator=g)
    km = torch.arange(sk).view(1, -1) < torch.randint(max(1, sk - 20), sk + 1, (b, 1), generator=g)
    qu, iq, cuq, mq, _ = unpad_input(q, qm)
    ku, _, cuk, mk, _ = unpad_input(k, km)
    vu = unpad_input(v, km)[0]
    out_u, lse, _ = fa.flash_attn_varlen_func(qu.to(DEV), ku.to(DEV), vu.to(DEV), cuq.to(DEV), cuk.to(DEV), mq, mk,
                                              causal=causal, return_attn_probs=True)
    out = pad_input(out_u.cpu(), iq, b, sq)
    out_ref, _ = oracle.attention_ref(q, k, v, qm, km, causal=causal)
    out_pt, _ = oracle.attention_ref(q, k, v, qm, km, causal=causal, upcast=False, reorder_ops=True)
    _check(out, out_ref, out_pt, f"varlen {sq}x{sk}")
    # lse (h, total_q) against the per-sequence oracle
    _, lse_ref = oracle.attention_varlen_ref(qu, ku, vu, cuq, cuk, causal=causal)
    _check_lse(lse, lse_ref)


def test_varlen_zero_length_sequences():
    """Zero-length key and query sequences inside a batch (hopper/test_flash_attn.py:388-433)."""
    fa = _api()
    torch.manual_seed(6)
    lens_q = [5, 0, 130, 64, 0]
    lens_k = [7, 33, 0, 300, 0]
    cuq = torch.tensor([0] + list(torch.tensor(lens_q).cumsum(0)), dtype=torch.int32)
    cuk = torch.tensor([0] + list(torch.tensor(lens_k).cumsum(0)), dtype=torch.int32)
    q = torch.randn(sum(lens_q), 4, 64, dtype=torch.bfloat16)
    k = torch.randn(sum(lens_k), 2, 64, dtype=torch.bfloat16)
    v = torch.randn(sum(lens_k), 2, 64, dtype=torch.bfloat16)
    out, lse, _ = fa.flash_attn_varlen_func(q.to(DEV), k.to(DEV), v.to(DEV), cuq.to(DEV), cuk.to(DEV),
                                            max(lens_q), max(lens_k), return_attn_probs=True)
    out_ref, lse_ref = oracle.attention_varlen_ref(q, k, v, cuq, cuk)
    out_pt, _ = oracle.attention_varlen_ref(q, k, v, cuq, cuk, upcast=False, reorder_ops=True)
    _check(out, out_ref, out_pt, "zero-length")
    # the sequence with queries but no keys: zero output rows, +inf lse
    assert torch.all(out[5:135] == 0)
    _check_lse(lse, lse_ref)


def test_strided_views_qkvpacked():
    """Packed QKV views (row stride 3*h*d) are read in place (flash_attn_interface.py:1008-1062)."""
    fa = _api()
    torch.manual_seed(7)
    qkv = torch.randn(2, 333, 3, 4, 128, dtype=torch.bfloat16)
    out = fa.flash_attn_qkvpacked_func(qkv.to(DEV), causal=True)
    out_ref, out_pt, _ = _dense_ref(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], causal=True)
    _check(out, out_ref, out_pt, "qkvpacked")


def test_forward_bitwise_deterministic():
    """out and lse bit-identical across repeated launches (tests/test_flash_attn.py:2199-2237)."""
    fa = _api()
    torch.manual_seed(8)
    q = torch.randn(2, 1024, 8, 128, dtype=torch.bfloat16, device=DEV)
    k = torch.randn(2, 1024, 8, 128, dtype=torch.bfloat16, device=DEV)
    v = torch.randn(2, 1024, 8, 128, dtype=torch.bfloat16, device=DEV)
    out0, lse0, _ = fa.flash_attn_func(q, k, v, causal=True, return_attn_probs=True)
    for _ in range(50):
        out, lse, _ = fa.flash_attn_func(q, k, v, causal=True, return_attn_probs=True)
        assert torch.equal(out, out0)
        assert torch.equal(lse, lse0)


def test_rescale_branch_forced():
    """A spike in one late key block forces the running-max rescale on rows that already hold
    accumulated output (cdna guide rule 26: the rare branch needs its own input)."""
    fa = _api()
    torch.manual_seed(9)
    sq, sk, d = 256, 1024, 128
    q = torch.randn(1, sq, 2, d, dtype=torch.bfloat16)
    k = torch.randn(1, sk, 2, d, dtype=torch.bfloat16)
    v = torch.randn(1, sk, 2, d, dtype=torch.bfloat16)
    k[0, 700] = q[0, 37] * 3.0      # key 700 (tile 10) dominates row 37 late in the sweep
    k[0, 1023] = q[0, 200] * 4.0    # last key dominates row 200
    out, lse, _ = fa.flash_attn_func(q.to(DEV), k.to(DEV), v.to(DEV), return_attn_probs=True)
    out_ref, out_pt, lse_ref = _dense_ref(q, k, v)
    _check(out, out_ref, out_pt, "forced rescale")
    _check_lse(lse, lse_ref, tol=5e-3)


@pytest.mark.parametrize("d", [128, 64])
def test_phantom_trip_forced(d):
    """Forces guard A / guard B of the generated loop to trip ON the phantom half-step: the block that runs a
    wave's last unmasked tile also forms the scores of the half-step BEHIND it, and behind the end of a split-KV range those
    are real keys.  A dominant key in the first 32 keys behind each split boundary makes the phantom's row sums (q-block A:
    rows r < 32 of a wave) or its look-ahead max (q-block B) overflow the stale max -- deterministically, not 2 seeds in 24.
    The same keys are ordinary keys of the next split, whose prologue must handle them; the merged result is compared
    with the oracle.  sq 512 = 2 m-blocks x 4 waves, sk 2048 in 4 splits of 8 tiles: boundaries at keys 512 / 1024 / 1536."""
    fa = _api()
    torch.manual_seed(31)
    sq, sk = 512, 2048
    q = torch.randn(1, sq, 4, d, dtype=torch.bfloat16)
    k = torch.randn(1, sk, 2, d, dtype=torch.bfloat16)
    v = torch.randn(1, sk, 2, d, dtype=torch.bfloat16)
    # (query row, key): rows 10 / 200 / 458 sit in a q-block A (row % 64 < 32), rows 300 / 120 in a q-block B
    spikes = [(10, 512 + 5), (300, 1024 + 20), (200, 1536 + 31), (458, 512 + 17), (120, 1536 + 0)]
    for i, (row, key) in enumerate(spikes):
        k[0, key, i % 2] = q[0, row, 2 * (i % 2)] * 3.0   # head 0 / 2 of GQA group i % 2
    out_ref, out_pt, lse_ref = _dense_ref(q, k, v)
    for splits in (4, 1):
        out, lse = fa.flash_attn_with_kvcache(q.to(DEV), k.to(DEV), v.to(DEV), num_splits=splits, return_softmax_lse=True)
        _check(out, out_ref, out_pt, f"phantom trip, num_splits={splits}")
        _check_lse(lse, lse_ref, tol=5e-3)


@pytest.mark.parametrize("d", [128, 64])
def test_block_boundary_trip_forced_causal(d):
    """The causal twin: a dominant key in the first (diagonal) tile behind a wave's last unmasked tile trips the guards in the
    LAST half-step of the unmasked generated block -- the exit where the generic half-step must redo P_A from the kept
    scores and hand over to the MASKED block -- for rows of q-block A and of q-block B, in every wave of two m-blocks."""
    fa = _api()
    torch.manual_seed(32)
    s = 2304                               # (> 2048: head dim 64 keeps the 256-row kernel under a causal mask)
    q = torch.randn(1, s, 2, d, dtype=torch.bfloat16)
    k = torch.randn(1, s, 2, d, dtype=torch.bfloat16)
    v = torch.randn(1, s, 2, d, dtype=torch.bfloat16)
    for mb in (2, 8):                      # m-blocks whose waves have >= 2 unmasked tiles in front of the diagonal
        for w in range(4):
            wrow = 256 * mb + 64 * w
            row = wrow + (10 if w % 2 == 0 else 45)          # q-block A / q-block B
            k[0, wrow + 2 + w, w % 2] = q[0, row, w % 2] * 3.0   # visible to `row` (key <= row), first half-step of the diagonal tile
    out, lse, _ = fa.flash_attn_func(q.to(DEV), k.to(DEV), v.to(DEV), causal=True, return_attn_probs=True)
    out_ref, out_pt, lse_ref = _dense_ref(q, k, v, causal=True)
    _check(out, out_ref, out_pt, "forced trip at the unmasked/masked block boundary")
    _check_lse(lse, lse_ref, tol=5e-3)


@pytest.mark.parametrize("d", [128, 64])
@pytest.mark.parametrize("variant", [0, 1, 2, 3])
def test_kernel_variants_agree(variant, d):
    """Every tile shape the dispatcher can pick gives the same answer as the oracle (0 = the library's policy, which
    sends short causal problems like this one to the 32-row shapes; 3 = the 256-row pipelined kernel regardless)."""
    from flash_attention_annotated_amd import _lib
    fa = _api()
    lib = _lib.load()
    torch.manual_seed(10)
    q = torch.randn(2, 777, 4, d, dtype=torch.bfloat16)
    k = torch.randn(2, 901, 2, d, dtype=torch.bfloat16)
    v = torch.randn(2, 901, 2, d, dtype=torch.bfloat16)
    out_ref, out_pt, _ = _dense_ref(q, k, v, causal=True)
    try:
        lib.fa_set_default_variant(variant)
        out = fa.flash_attn_func(q.to(DEV), k.to(DEV), v.to(DEV), causal=True)
    finally:
        lib.fa_set_default_variant(0)
    _check(out, out_ref, out_pt, f"variant {variant}")


def test_full_size_properties_c2():
    """BASELINE config 2 (b4 h16 s8192 d128 bf16) at full size through size-independent properties:
    (1) a 2-row x all-heads slice equals the oracle computed for those rows only;
    (2) softmax convexity: every output lies inside [min V, max V] of its kv head;
    (3) permuting the keys (and values alike) leaves lse unchanged up to fp32 rounding."""
    fa = _api()
    torch.manual_seed(0)
    b, s, h, d = 4, 8192, 16, 128
    q = torch.randn(b, s, h, d, dtype=torch.bfloat16, device=DEV)
    k = torch.randn(b, s, h, d, dtype=torch.bfloat16, device=DEV)
    v = torch.randn(b, s, h, d, dtype=torch.bfloat16, device=DEV)
    out, lse, _ = fa.flash_attn_func(q, k, v, return_attn_probs=True)
    assert torch.isfinite(out.float()).all()
    rows = [0, 4097, 8191]
    qs = q[:, rows].cpu()
    out_ref, out_pt, lse_ref = _dense_ref(qs, k.cpu(), v.cpu())
    _check(out[:, rows], out_ref, out_pt, "c2 slice")
    _check_lse(lse[:, :, rows], lse_ref)
    vmin = v.float().amin(dim=1, keepdim=True)
    vmax = v.float().amax(dim=1, keepdim=True)
    assert (out.float() >= vmin - 1e-2).all() and (out.float() <= vmax + 1e-2).all()
    perm = torch.randperm(s, device=DEV)
    out2, lse2, _ = fa.flash_attn_func(q[:1], k[:1, perm], v[:1, perm], return_attn_probs=True)
    assert (lse2 - lse[:1]).abs().max().item() < 1e-3
    assert (out2.float() - out[:1].float()).abs().max().item() < 2e-2


def test_error_messages():
    fa = _api()
    q = torch.randn(1, 8, 2, 64, dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError, match="only support fp16 and bf16"):
        fa.flash_attn_func(q, q, q)
    q = torch.randn(1, 8, 3, 64, dtype=torch.bfloat16, device=DEV)
    k = torch.randn(1, 8, 2, 64, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="must divide number of heads in query"):
        fa.flash_attn_func(q, k, k)
    q = torch.randn(1, 8, 2, 264, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="at most 256"):
        fa.flash_attn_func(q, q, q)


def test_empty_keys_dense():
    """seqlen_k == 0: out = 0, lse = +inf (csrc/flash_attn/flash_api.cpp:499-504)."""
    fa = _api()
    q = torch.randn(1, 8, 2, 64, dtype=torch.bfloat16, device=DEV)
    k = torch.empty(1, 0, 2, 64, dtype=torch.bfloat16, device=DEV)
    out, lse, _ = fa.flash_attn_func(q, k, k, return_attn_probs=True)
    assert torch.all(out == 0) and torch.all(torch.isposinf(lse))


def _sweep_form(feature, d, causal):
    """The kernel a problem of test_row_block_kernel_random_sweep runs when it does not reach fwd_kernel_d256 (plan_fwd: every
    seed is split by the FA2 heuristic, and a split problem stays in the 256-row kernel at head dims <= 128 -- the 4-wave
    compiler-scheduled shape for a causal problem at head dim <= 64 -- and runs the compiler-scheduled shape above 128)."""
    cap = " SOFTCAP" if feature == "softcap" else ""
    if d > 128:
        return "fwd_kernel D=256 waves=4" + cap
    if d <= 64:
        return ("fwd_kernel D=64 waves=4" if causal else "fwd_kernel_w64 D=64 DEFF=64 waves=4") + cap
    return f"fwd_kernel_w64 D=128 DEFF={96 if d <= 96 and not cap else 128} waves=4" + cap


@pytest.mark.parametrize("seed", list(range(24)))
def test_row_block_kernel_random_sweep(seed):
    """Seeded random problems over what the 32-row-per-wave kernel (fa_fwd_kernel_d256.h) takes since round 3: head dims
    40 .. 256 with softcap or ALiBi, head dims 136 .. 256 plain, causal / windows / neither, GQA, odd lengths, both 16-bit
    types -- unmasked body, masked body (diagonal, ragged tail, last tile) and the generic half-step (left window edge, guard
    trips) in one sweep each; out and LSE against the oracle.  What it reaches is less than that: batch 2 x at most 6 heads
    is few enough work items for the FA2 entry point's split-KV heuristic to split every one of the 24 seeds (planned on 256
    CUs), and a split problem never runs fwd_kernel_d256 -- head dims <= 128 stay in the 256-row kernel (fwd_kernel_w64, plain
    or SOFTCAP), head dims above run the compiler-scheduled shape (fwd_kernel D=256 waves=4); an unsplit causal problem at head
    dim <= 64 with seqlen_k <= 2048 would run fwd_kernel D=64 waves=4, not fwd_kernel_d256 W=64.  The sweep keeps its problems
    (what it covers today stays covered) and asserts and prints the plan of every seed; the fwd_kernel_d256 forms are covered
    by name in tests/test_plan_parity_gpu.py."""
    fa = _api()
    g = torch.Generator().manual_seed(1000 + seed)
    ri = lambda lo, hi: int(torch.randint(lo, hi + 1, (1,), generator=g).item())
    feature = ("softcap", "alibi", "plain")[seed % 3]
    d = 8 * ri(17, 32) if feature == "plain" else 8 * ri(5, 32)
    dtype = (torch.bfloat16, torch.float16)[ri(0, 1)]
    sq, sk = ri(300, 1200), ri(600, 1500)
    if ri(0, 2) == 0:
        sq = sk
    hk = ri(1, 2)
    h = hk * ri(1, 3)
    mask = ri(0, 3)
    kw = dict(causal=True) if mask == 1 else (dict(window_size=(ri(50, 700), ri(0, 200))) if mask == 2 else
                                              (dict(window_size=(ri(100, 500), -1)) if mask == 3 else {}))
    q = torch.randn(2, sq, h, d, generator=g).to(dtype)
    k = torch.randn(2, sk, hk, d, generator=g).to(dtype)
    v = torch.randn(2, sk, hk, d, generator=g).to(dtype)
    okw = dict(kw)
    if "window_size" in kw and kw["window_size"][1] < 0:
        okw["window_size"] = (kw["window_size"][0], sk)   # (the FA2 entry point's mirror rule, csrc/flash_attn/flash_api.cpp:141-142)
    if feature == "softcap":
        kw["softcap"] = okw["softcap"] = 12.0 + ri(0, 30)
        q = q * (kw["softcap"] / 4)
    elif feature == "alibi":
        slopes = torch.rand(2, h, generator=g) * 0.05   # (small slopes: the block is not left at every tile)
        kw["alibi_slopes"] = slopes.to(DEV)
        okw["attn_bias"] = oracle.attn_bias_from_alibi_slopes(slopes, sq, sk, causal=False)
    out, lse, _ = fa.flash_attn_func(q.to(DEV), k.to(DEV), v.to(DEV), return_attn_probs=True, **kw)
    plan = last_plan()
    print(f"seed {seed}: {feature} d{d} {sq}x{sk} {sorted(kw)} -> {plan}")
    assert plan.startswith(("fwd_kernel_d256 W=", _sweep_form(feature, d, mask == 1) + " block_m=")), plan
    out_ref, out_pt, lse_ref = _dense_ref(q, k, v, **okw)
    err = (out.float().cpu() - out_ref.float()).abs().max().item()
    bound = 3 * (out_pt.float() - out_ref.float()).abs().max().item() + 2 * (out_ref + 0.3 - 0.3 - out_ref).abs().max().item() + 1e-5
    assert err <= bound, (feature, d, sq, sk, kw.keys(), err, bound)
    _check_lse(lse, lse_ref, tol=5e-3)
