"""GPU tests of the fused dropout + residual-add + LayerNorm / RMSNorm (flash_attention_annotated_amd.ops.layer_norm over
csrc/fa_dropout_norm.hip).

Parity is taken *given the mask*: the call returns its dropout mask, the oracle (ops.norm.layer_norm_ref / rms_norm_ref) runs
with that mask in fp64 and again in the operands' dtypes, and every forward output and every gradient must satisfy the
contract of tests/test_norm_gpu.py with its constants:  max|ours - ref64| <= 2 max|ref_in_dtype - ref64| + atol,  atol 5e-2
with bf16 among the dtypes, 1e-2 with fp16, 1e-4 in fp32.  The backward stores no mask: that its gradients agree with the
oracle under the returned mask shows that it draws the same decisions again.
"""
import random

import pytest
import torch
import torch.nn.functional as F

import dropout_norm_plan_universe as U
from flash_attention_annotated_amd.ops import layer_norm as L
from flash_attention_annotated_amd.ops import norm
from flash_attention_annotated_amd.ops.triton.layer_norm import layer_norm_fn

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, FP16, FP32 = torch.bfloat16, torch.float16, torch.float32
DT = {"bf16": BF16, "fp16": FP16, "fp32": FP32}
EPS = 1e-5


def atol_of(*dtypes):
    return 5e-2 if BF16 in dtypes else 1e-2 if FP16 in dtypes else 1e-4


def accept(name, ours, pt, ref, atol):
    """max|ours - ref64| <= 2 max|ref_in_dtype - ref64| + atol"""
    err = (ours.double() - ref.double()).abs().max().item() if ours.numel() else 0.0
    base = (pt.double() - ref.double()).abs().max().item() if ours.numel() else 0.0
    print(f"{name}: err {err:.3e} bound 2 * {base:.3e} + {atol:g}")
    assert err <= 2 * base + atol, f"{name}: {err} > 2 * {base} + {atol}"


def grid_drop_fraction(p):
    """an element is kept iff its byte <= floor(255 (1 - p)): the drop probability on the 8-bit grid"""
    return 1 - (int(255 * (1 - p)) + 1) / 256


def _leaves(ts, dtype=None):
    return [t.detach().to(dtype or t.dtype).clone().requires_grad_(True) if t is not None else None for t in ts]


def _oracle(rms, leaves, rowscale, p, prenorm, masks, two):
    x0, x1, res, w0, b0, w1, b1, cs = leaves
    ref = norm.rms_norm_ref if rms else norm.layer_norm_ref
    # (the layerscale enters by pre-multiplying, in x0's dtype: the oracle keeps the stream in the dtype of what it is given, and
    # a product promoted to an fp32 layerscale's dtype would leave the stream of a 16-bit x0 unrounded)
    out = ref((x0 * cs).to(x0.dtype) if cs is not None else x0, w0, b0, residual=res, x1=x1, weight1=w1, bias1=b1, eps=EPS, dropout_p=p,
              rowscale=rowscale.to(x0.dtype) if rowscale is not None else None, prenorm=prenorm, dropout_mask=masks[0],
              dropout_mask1=masks[1])
    out = out if isinstance(out, tuple) else (out,)
    zs, x = (out[:-1], out[-1]) if prenorm else (out, None)
    return zs[0], (zs[1] if two else None), x


def check(rms, x0, w0, b0=None, res=None, x1=None, w1=None, b1=None, rowscale=None, colscale=None, p=0.0, prenorm=False,
          r32=False, parallel=False, backward=True):
    """One call against the oracle given the mask it returned; -> (dmask0, dmask1, outputs of ours)."""
    parallel = parallel or x1 is not None or w1 is not None
    two = w1 is not None
    tensors = (x0, x1, res, w0, b0, w1, b1, colscale)
    ours, pt, ref = _leaves(tensors), _leaves(tensors), _leaves(tensors, torch.float64)
    a = ours
    if parallel:
        fn = L.dropout_add_rms_norm_parallel_residual if rms else L.dropout_add_layer_norm_parallel_residual
        out = fn(a[0], a[1], a[2], a[3], a[4], a[5], a[6], p, EPS, prenorm=prenorm, residual_in_fp32=r32, return_dropout_mask=True)
        z0, z1 = out[0], out[1]
        x = out[2] if prenorm else None
        dmask0, dmask1 = out[-2], out[-1]
        assert (z1 is None) == (not two)
    else:
        fn = L.dropout_add_rms_norm if rms else L.dropout_add_layer_norm
        out = fn(a[0], a[2], a[3], a[4], p, EPS, rowscale=rowscale, layerscale=a[7], prenorm=prenorm, residual_in_fp32=r32,
                 return_dropout_mask=True)
        z0, z1, x, dmask0, dmask1 = out[0], None, out[1] if prenorm else None, out[-1], None
    assert len(out) == (2 if parallel else 1) + int(prenorm) + (2 if parallel else 1)
    stream_dtype = res.dtype if res is not None else FP32 if r32 else x0.dtype
    atol = atol_of(x0.dtype, w0.dtype, stream_dtype)
    for m in (dmask0, dmask1):
        if m is not None:
            assert m.dtype == torch.uint8 and m.shape == x0.shape and int(m.max()) <= 1 if m.numel() else True
    if p == 0.0 or x1 is None:
        assert dmask1 is None or bool(dmask1.all())
    if p == 0.0:
        assert bool(dmask0.all())
    masks = (dmask0.bool(), dmask1.bool() if dmask1 is not None else None)
    z0_pt, z1_pt, x_pt = _oracle(rms, pt, rowscale, p, prenorm, masks, two)
    z0_ref, z1_ref, x_ref = _oracle(rms, ref, rowscale.double() if rowscale is not None else None, p, prenorm, masks, two)
    assert z0.dtype == x0.dtype and z0.shape == x0.shape
    accept("z0", z0, z0_pt, z0_ref, atol)
    if two:
        accept("z1", z1, z1_pt, z1_ref, atol)
    if prenorm:
        assert x.dtype == stream_dtype and x.shape == x0.shape
        accept("x", x, x_pt, x_ref, atol)
    if not backward:
        return dmask0, dmask1, out
    g = torch.randn_like(z0_pt) / 8
    g1 = torch.randn_like(z0_pt) / 8

    def loss(z0_, z1_, x_, cast):
        t = z0_ * g.to(z0_.dtype)
        if two:
            t = t + z1_ * g1.to(z1_.dtype)
        if prenorm:
            t = t * F.sigmoid(x_.to(cast) if cast else x_)
        return t.sum()
    loss(z0, z1, x, None).backward()
    loss(z0_pt, z1_pt, x_pt, None).backward()
    loss(z0_ref, z1_ref, x_ref.to(stream_dtype) if prenorm else None, torch.float64).backward()
    names = ("dx0", "dx1", "dresidual", "dw0", "db0", "dw1", "db1", "dcolscale")
    for name, o, q, r in zip(names, ours, pt, ref):
        if o is None:
            continue
        assert o.grad is not None and o.grad.dtype == o.dtype and o.grad.shape == o.shape, name
        accept(name, o.grad, q.grad, r.grad, atol)
    return dmask0, dmask1, out


def operands(m, n, x0_dtype, w_dtype, res, rms, form, bias, seed, shape=None):
    """res: None / "same" / "fp32"; form: one of U.FORMS"""
    torch.manual_seed(seed)
    shape = shape or (m, n)
    x0 = torch.randn(*shape, device=DEV, dtype=x0_dtype)
    kw = dict(w0=torch.randn(n, device=DEV, dtype=w_dtype))
    if bias:
        kw["b0"] = torch.randn(n, device=DEV, dtype=w_dtype)
    if res:
        kw["res"] = torch.randn(*shape, device=DEV, dtype=FP32 if res == "fp32" else x0_dtype)
    if form == "scaled":
        kw["rowscale"] = torch.rand(shape[:-1], device=DEV, dtype=x0_dtype) + 0.5
        kw["colscale"] = torch.randn(n, device=DEV, dtype=w_dtype)
    if form in ("parallel", "parallel_no_x1", "two_weights_no_x1_no_res"):
        kw["w1"] = torch.randn(n, device=DEV, dtype=w_dtype)
        kw["parallel"] = True
        if bias:
            kw["b1"] = torch.randn(n, device=DEV, dtype=w_dtype)
    if form == "parallel":
        kw["x1"] = torch.randn(*shape, device=DEV, dtype=x0_dtype)
    return x0, kw


# ---- every universe case: every kernel, both sides of every plan boundary ----------------------------------------------------
@pytest.mark.parametrize("c", U.CASES, ids=U.case_id)
def test_universe_case(c):
    x0, kw = operands(c.m, c.n, DT[c.x0], DT[c.w], c.res, c.rms, c.form, c.bias, c.n)
    args = L._forward_args(x0, kw.get("x1"), kw.get("res"), kw["w0"], kw.get("b0"), kw.get("w1"), kw.get("b1"), kw.get("rowscale"),
                           kw.get("colscale"), c.p, EPS, c.r32, c.rms, c.prenorm, True)
    assert U.form_of_plan(L._plan_forward(x0, kw.get("x1"), kw.get("res"), kw["w0"], kw.get("b0"), kw.get("w1"), kw.get("b1"),
                                          kw.get("rowscale"), kw.get("colscale"), c.p, EPS, c.r32, c.rms, c.prenorm, True)) == \
        U.form_of("fwd", c), args[9:]
    check(c.rms, x0, p=c.p, prenorm=c.prenorm, r32=c.r32, **kw)


# ---- the grid: a seeded subset of the product, every value of every axis, every (N, p) -----------------------------------------
NS = (8, 24, 264, 1024, 8192, 203)
PS = (0.0, 0.17, 0.9)
AXES = dict(m=(1, 3, 33), rms=(False, True), res=(None, "same", "fp32"), r32=(False, True), prenorm=(False, True),
            form=U.FORMS, bias=(False, True), x0=(BF16, FP16, FP32), w=(BF16, FP16, FP32))


def _grid():
    rng = random.Random(20261020)
    cases = []
    for n in NS:
        for p in PS:
            for _ in range(2):
                c = {k: rng.choice(v) for k, v in AXES.items()}
                if c["x0"] == FP32 and c["res"] == "same":
                    c["res"] = "fp32"
                c.update(n=n, p=p)
                cases.append(c)
    return cases


GRID = _grid()
SHORT = {BF16: "bf16", FP16: "fp16", FP32: "fp32"}


def _gid(c):
    return (f"m{c['m']}-n{c['n']}-p{c['p']:g}-{'rms' if c['rms'] else 'ln'}-{c['form']}-{SHORT[c['x0']]}-w{SHORT[c['w']]}"
            f"-res_{c['res']}{'-r32' if c['r32'] else ''}{'-pre' if c['prenorm'] else ''}{'-b' if c['bias'] else ''}")


def test_grid_covers_every_axis_value():
    for axis, values in AXES.items():
        assert {c[axis] for c in GRID} == set(values), axis
    assert {(c["n"], c["p"]) for c in GRID} == {(n, p) for n in NS for p in PS}
    triples = {(c["x0"], FP32 if c["res"] == "fp32" else c["x0"], c["w"]) for c in GRID}
    assert {t[0] for t in triples} == {t[2] for t in triples} == {BF16, FP16, FP32}


@pytest.mark.parametrize("c", GRID, ids=_gid)
def test_parity_given_the_mask(c):
    x0, kw = operands(c["m"], c["n"], c["x0"], c["w"], c["res"], c["rms"], c["form"], c["bias"], c["n"] + c["m"])
    check(c["rms"], x0, p=c["p"], prenorm=c["prenorm"], r32=c["r32"], **kw)


@pytest.mark.parametrize("rms", [False, True], ids=["ln", "rms"])
@pytest.mark.parametrize("form", ["scaled", "parallel"])
def test_strided_and_3d_inputs(form, rms):
    """(2, 7, N) views with a row pitch of 2 N: x0, x1 and the residual are read in place; dz arrives strided too"""
    n = 264
    torch.manual_seed(5)
    x0, kw = operands(14, n, BF16, FP32, "fp32", rms, form, True, 7, shape=(2, 7, 2 * n))
    x0 = x0[..., :n]
    for k in ("res", "x1"):
        if k in kw:
            kw[k] = kw[k][..., :n]
    assert not x0.is_contiguous()
    check(rms, x0, p=0.17, prenorm=True, **kw)


@pytest.mark.parametrize("parallel", [False, True], ids=["one_weight", "parallel"])
def test_no_rows(parallel):
    n = 24
    x0 = torch.randn(0, n, device=DEV, dtype=BF16, requires_grad=True)
    w = torch.randn(n, device=DEV, dtype=BF16, requires_grad=True)
    b = torch.randn(n, device=DEV, dtype=BF16, requires_grad=True)
    if parallel:
        z0, z1, x, m0, m1 = L.dropout_add_layer_norm_parallel_residual(x0, None, None, w, b, w, b, 0.1, EPS, prenorm=True,
                                                                       return_dropout_mask=True)
        assert z1.shape == (0, n) and m1.shape == (0, n)
    else:
        z0, x, m0 = L.dropout_add_layer_norm(x0, None, w, b, 0.1, EPS, prenorm=True, return_dropout_mask=True)
    assert z0.shape == x.shape == m0.shape == (0, n) and m0.dtype == torch.uint8
    (z0.sum() + x.sum()).backward()
    assert x0.grad.shape == (0, n) and not w.grad.any() and not b.grad.any()


# ---- the mask itself -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.05, 0.17, 0.5, 0.9])
def test_drop_fraction_is_on_the_8_bit_grid(p):
    """2^20 decisions: the sampling deviation is below 0.001, the margin DESIGN 4.6's own 0.01"""
    x0 = torch.randn(1024, 1024, device=DEV, dtype=BF16)
    w = torch.ones(1024, device=DEV, dtype=BF16)
    _, m0, m1 = L.dropout_add_layer_norm_parallel_residual(x0, x0, None, w, None, None, None, p, EPS, return_dropout_mask=True)[1:]
    for m in (m0, m1):
        drop = 1 - m.float().mean().item()
        print(f"p {p}: dropped {drop:.5f}, grid {grid_drop_fraction(p):.5f}")
        assert abs(drop - grid_drop_fraction(p)) < 0.01
    assert not torch.equal(m0, m1)  # the two streams draw their own decisions
    assert not torch.equal(m0[0], m0[1])  # ... and so do two rows


def test_seed_reproduces_the_mask_and_calls_advance_it():
    x0 = torch.randn(33, 264, device=DEV, dtype=FP16)
    w = torch.ones(264, device=DEV, dtype=FP16)

    def call():
        return L.dropout_add_layer_norm(x0, None, w, None, 0.17, EPS, return_dropout_mask=True)
    torch.manual_seed(11)
    z_a, m_a = call()
    z_b, m_b = call()
    torch.manual_seed(11)
    z_c, m_c = call()
    assert torch.equal(m_a, m_c) and torch.equal(z_a, z_c)
    assert not torch.equal(m_a, m_b)


def test_column_sums_are_bit_equal_over_two_backward_calls():
    """slabs and an ordered reduce, no atomics: dw, db and dcolscale of two runs of the same backward are the same bits"""
    torch.manual_seed(3)
    x0, kw = operands(333, 1040, BF16, FP32, "fp32", False, "scaled", True, 3)
    grads = []
    for _ in range(2):
        leaves = _leaves((x0, kw["res"], kw["w0"], kw["b0"], kw["colscale"]))
        torch.manual_seed(4)
        z, x = L.dropout_add_layer_norm(leaves[0], leaves[1], leaves[2], leaves[3], 0.17, EPS, rowscale=kw["rowscale"],
                                        layerscale=leaves[4], prenorm=True)
        torch.manual_seed(5)
        (z.float() * torch.randn_like(z, dtype=FP32) + x.sin()).sum().backward()
        grads.append([t.grad for t in leaves])
    for a, b in zip(*grads):
        assert torch.equal(a, b)
    x0, kw = operands(333, 1040, BF16, BF16, None, True, "parallel", True, 3)
    grads = []
    for _ in range(2):
        leaves = _leaves((x0, kw["x1"], kw["w0"], kw["b0"], kw["w1"], kw["b1"]))
        torch.manual_seed(4)
        z0, z1 = L.dropout_add_rms_norm_parallel_residual(leaves[0], leaves[1], None, leaves[2], leaves[3], leaves[4], leaves[5], 0.17,
                                                          EPS)
        (z0.float().sin() + z1.float().cos()).sum().backward()
        grads.append([t.grad for t in leaves])
    for a, b in zip(*grads):
        assert torch.equal(a, b)


def test_past_2_31_elements():
    """M N = 2^31 + 3 N: rows are addressed, and decisions drawn, in 64 bits.  The last 1024 rows match the oracle given the
    mask, their drop fraction is on the grid, and their mask is not that of the first 1024 rows."""
    m, n, p = (1 << 18) + 3, 8192, 0.17
    torch.manual_seed(0)
    x0 = torch.randn(m, n, device=DEV, dtype=BF16)
    w = torch.randn(n, device=DEV, dtype=BF16)
    b = torch.randn(n, device=DEV, dtype=BF16)
    z, mask = L.dropout_add_layer_norm(x0, None, w, b, p, EPS, return_dropout_mask=True)
    assert z.shape == mask.shape == (m, n)
    tail, tmask = slice(m - 1024, m), mask[m - 1024:].bool()
    z_pt = norm.layer_norm_ref(x0[tail], w, b, eps=EPS, dropout_p=p, dropout_mask=tmask)
    z_ref = norm.layer_norm_ref(x0[tail].double(), w.double(), b.double(), eps=EPS, dropout_p=p, dropout_mask=tmask)
    accept("z tail", z[tail], z_pt, z_ref, atol_of(BF16))
    drop = 1 - tmask.float().mean().item()
    assert abs(drop - grid_drop_fraction(p)) < 0.01
    assert not torch.equal(mask[:1024], mask[m - 1024:])


# ---- graphs, compile, modules ----------------------------------------------------------------------------------------------------
def test_graph_capture_and_replay():
    n = 1024
    x0 = torch.randn(33, n, device=DEV, dtype=BF16)
    res = torch.randn(33, n, device=DEV, dtype=FP32)
    w = torch.randn(n, device=DEV, dtype=BF16)
    b = torch.randn(n, device=DEV, dtype=BF16)

    def call():
        return L.dropout_add_layer_norm(x0, res, w, b, 0.17, EPS, prenorm=True, return_dropout_mask=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        z, x, mask = call()
    runs = []
    for seed in (21, 21, None):
        if seed is not None:
            torch.manual_seed(seed)
        graph.replay()
        runs.append((z.clone(), x.clone(), mask.clone()))
    assert torch.equal(runs[0][2], runs[1][2]) and torch.equal(runs[0][0], runs[1][0])  # re-seeded: the same decisions
    assert not torch.equal(runs[1][2], runs[2][2])  # replayed on: new ones
    for z_, x_, mask_ in runs[1:]:  # what a replay wrote is what eager computes given its mask
        kw = dict(residual=res, eps=EPS, dropout_p=0.17, prenorm=True, dropout_mask=mask_.bool())
        z_pt, x_pt = norm.layer_norm_ref(x0, w, b, **kw)
        z_ref, x_ref = norm.layer_norm_ref(x0.double(), w.double(), b.double(), **{**kw, "residual": res.double()})
        accept("z", z_, z_pt, z_ref, atol_of(BF16))
        accept("x", x_, x_pt, x_ref, atol_of(BF16))
        drop = 1 - mask_.float().mean().item()
        assert abs(drop - grid_drop_fraction(0.17)) < 0.02  # (33 * 1024 decisions: a deviation of 0.002)


def _train_check(mod, rms, compiled=None):
    """prenorm and no residual: the stream is zero exactly where x0 was dropped, which is the mask"""
    n = mod.weight.numel()
    torch.manual_seed(9)
    x0 = torch.randn(64, n, device=DEV, dtype=BF16, requires_grad=True)
    with torch.no_grad():
        mod.weight.normal_()
        if mod.bias is not None:
            mod.bias.normal_()
    z, x = (mod if compiled is None else compiled)(x0)
    mask = x != 0
    drop = 1 - mask.float().mean().item()
    assert abs(drop - grid_drop_fraction(mod.p)) < 0.01  # (2^16 decisions: a deviation of 0.002)
    g = torch.randn_like(z)
    (z * g).sum().backward()
    ref = norm.rms_norm_ref if rms else norm.layer_norm_ref
    outs = []
    for dtype in (BF16, torch.float64):
        xl, wl, bl = _leaves((x0, mod.weight, mod.bias), dtype)
        zr, _ = ref(xl, wl, bl, eps=mod.eps, dropout_p=mod.p, prenorm=True, dropout_mask=mask)
        (zr * g.to(dtype)).sum().backward()
        outs.append((zr, xl.grad, wl.grad, bl.grad if bl is not None else None))
    ours = (z, x0.grad, mod.weight.grad, mod.bias.grad if mod.bias is not None else None)
    for name, o, q, r in zip(("z", "dx0", "dw", "db"), ours, *outs):
        if o is not None:
            accept(name, o, q, r, atol_of(BF16))


@pytest.mark.parametrize("rms", [False, True], ids=["ln", "rms"])
def test_module_train_mode(rms):
    cls = L.DropoutAddRMSNorm if rms else L.DropoutAddLayerNorm
    _train_check(cls(1024, prenorm=True, p=0.5, device=DEV, dtype=BF16).train(), rms)


@pytest.mark.parametrize("rms", [False, True], ids=["ln", "rms"])
@pytest.mark.parametrize("n", [1024, 4096])
def test_module_eval_mode_is_layer_norm_fn(n, rms):
    """No dropout, a 16-bit x0 in the 16-byte form and an fp32 stream: the sums of ops.triton.layer_norm in the same order,
    hence the same bits"""
    cls = L.DropoutAddRMSNorm if rms else L.DropoutAddLayerNorm
    mod = cls(n, prenorm=True, p=0.5, residual_in_fp32=True, device=DEV, dtype=BF16).eval()
    with torch.no_grad():
        mod.weight.normal_()
        if mod.bias is not None:
            mod.bias.normal_()
    x0 = torch.randn(33, n, device=DEV, dtype=BF16)
    res = torch.randn(33, n, device=DEV, dtype=FP32)
    for r in (res, None):
        z, x = mod(x0, r)
        z_ref, x_ref = layer_norm_fn(x0, mod.weight, mod.bias, residual=r, eps=mod.eps, prenorm=True, residual_in_fp32=True,
                                     is_rms_norm=rms)
        assert x.dtype == FP32 and torch.equal(x, x_ref) and torch.equal(z, z_ref)


def test_compile_fullgraph():
    mod = L.DropoutAddLayerNorm(1024, prenorm=True, p=0.5, device=DEV, dtype=BF16).train()
    _train_check(mod, False, compiled=torch.compile(mod, fullgraph=True))
