"""The oracle of csrc/fa_dropout_norm.hip for tests/test_dropout_norm_forms_gpu.py: the dropout decisions restated in integer
torch ops, and the forward and the backward of DESIGN 4.26's contract in plain torch, the masks being arguments.  Pure torch, no
library: it runs on the CPU (tests/test_dropout_norm_oracle.py) and on the device.

The functions compute in `dtype`: torch.float64 is the reference; torch.float32 is torch's eager evaluation of the same
formulas, which the bounds of the GPU tests are measured against.
"""
import torch

M32 = 0xFFFFFFFF


def keep_max(p):
    """an element is kept iff its byte <= keep_max: the keep probability on the 8-bit grid"""
    return int(255.0 * (1.0 - p))


def _mul32(x, c):
    """(x * c) mod 2^32 for an int64 tensor of 32-bit values and a 32-bit constant: no product passes 2^48"""
    return (x * (c & 0xFFFF) + (((x * (c >> 16)) & 0xFFFF) << 16)) & M32


def lowbias32(x):
    x = x ^ (x >> 16)
    x = _mul32(x, 0x7FEB352D)
    x = x ^ (x >> 15)
    x = _mul32(x, 0x846CA68B)
    return x ^ (x >> 16)


def seed_mix(seed, offset):
    """rng_state = {seed, offset} as one 32-bit word (csrc/fa_rowwise.h); Python integers"""
    seed, offset = seed & 0xFFFFFFFFFFFFFFFF, offset & 0xFFFFFFFFFFFFFFFF
    x = (seed & M32) ^ ((seed >> 32) * 0x27D4EB2F & M32) ^ ((offset & M32) * 0xC2B2AE3D & M32) ^ (offset >> 32)
    x ^= x >> 15
    x = (x * 0x2C1B3C6D) & M32
    return x ^ (x >> 12)


def row_key(mix, rows, stream):
    """the key of (row, stream); rows: an int64 tensor of row indices, the 64 bits split in two"""
    lo, hi = rows & M32, (rows >> 32) & M32
    return lowbias32((mix ^ _mul32(hi, 0x2545F491) ^ ((stream * 0x68E31DA4) & M32)) ^ _mul32(lo, 0x9E3779B1))


def group_bytes(key, g):
    """the word of column group g (columns 4 g .. 4 g + 3) under `key`: byte i decides column 4 g + i"""
    return lowbias32(key ^ ((_mul32(g, 0x85EBCA77) + 0x165667B1) & M32))


def mask_ref(seed, offset, m, n, stream, p, row0=0, device="cpu"):
    """uint8 (m, n), 1 = kept: the decisions of rows row0 .. row0 + m - 1 of stream 0 (x0) or 1 (x1) under rng_state =
    (seed, offset)"""
    rows = torch.arange(row0, row0 + m, dtype=torch.int64, device=device)
    key = row_key(seed_mix(seed, offset), rows, stream)
    g = torch.arange(-(-n // 4), dtype=torch.int64, device=device)
    word = group_bytes(key[:, None], g[None, :])
    byte = (word[:, :, None] >> (8 * torch.arange(4, dtype=torch.int64, device=device))) & 255
    return (byte.reshape(m, -1)[:, :n] <= keep_max(p)).to(torch.uint8)


def _to(t, dtype):
    return t.to(dtype) if t is not None else None


def stream_terms(x0, x1=None, residual=None, rowscale=None, colscale=None, p=0.0, keep0=None, keep1=None, dtype=torch.float64):
    """the terms the stream is the sum of, in the order they are added:
    keep0 * x0 * rowscale * colscale / (1 - p), keep1 * x1 / (1 - p), residual"""
    t = x0.to(dtype)
    if rowscale is not None:
        t = t * rowscale.to(dtype)[:, None]
    if colscale is not None:
        t = t * colscale.to(dtype)
    if p > 0.0:
        t = t * keep0.to(dtype) * (1.0 / (1.0 - p))
    terms = [t]
    if x1 is not None:
        terms.append(x1.to(dtype) * keep1.to(dtype) * (1.0 / (1.0 - p)) if p > 0.0 else x1.to(dtype))
    if residual is not None:
        terms.append(residual.to(dtype))
    return terms


def statistics(x, eps, rms, dtype=torch.float64):
    """mu (zeros for RMS) and rsigma of the rows of x"""
    x = x.to(dtype)
    mu = torch.zeros(x.shape[0], dtype=dtype, device=x.device) if rms else x.mean(-1)
    return mu, 1 / torch.sqrt(((x - mu[:, None]) ** 2).mean(-1) + eps)


def forward_ref(x0, w0, b0=None, x1=None, residual=None, w1=None, b1=None, rowscale=None, colscale=None, p=0.0, keep0=None,
                keep1=None, eps=1e-5, rms=False, x=None, dtype=torch.float64):
    """-> dict: x (the stream, not rounded), a (the sum of the absolute values of the terms added), mu, rsigma, z0, z1.
    With `x` the statistics and z0 / z1 are those of that stream, the one a kernel returned, not of the oracle's own."""
    terms = stream_terms(x0, x1, residual, rowscale, colscale, p, keep0, keep1, dtype)
    own, a = terms[0], terms[0].abs()
    for t in terms[1:]:
        own, a = own + t, a + t.abs()
    s = own if x is None else x.to(dtype)
    mu, rsigma = statistics(s, eps, rms, dtype)
    xhat = (s - mu[:, None]) * rsigma[:, None]

    def z(w, b):
        return xhat * w.to(dtype) + (b.to(dtype) if b is not None else 0.0)
    return dict(x=own, a=a, mu=mu, rsigma=rsigma, xhat=xhat, z0=z(w0, b0), z1=z(w1, b1) if w1 is not None else None)


def backward_ref(x, mu, rsigma, dz0, w0, dz1=None, w1=None, dx=None, x0=None, rowscale=None, colscale=None, p=0.0, keep0=None,
                 keep1=None, has_x1=False, rms=False, dtype=torch.float64):
    """The backward given the saved stream x, mu (None for RMS), rsigma, the gradients dz0 (dz1) of the outputs and dx of the
    stream (prenorm) -> dict of dresidual, dx0, dx1, dcolscale, dw0, db0, dw1, db1 (None where there is none) and the terms of
    their bounds t, t_dx0, t_dx1, t_dw0, t_db0, t_dw1, t_db1, t_dcolscale."""
    x, rs = x.to(dtype), rsigma.to(dtype)[:, None]
    xhat = (x - mu.to(dtype)[:, None]) * rs if not rms else x * rs
    wdz = w0.to(dtype) * dz0.to(dtype)
    if w1 is not None:
        wdz = wdz + w1.to(dtype) * dz1.to(dtype)
    c1 = (xhat * wdz).mean(-1, keepdim=True)
    c2 = torch.zeros_like(c1) if rms else wdz.mean(-1, keepdim=True)
    dxs = (wdz - xhat * c1 - c2) * rs
    t = rs * (wdz.abs() + xhat.abs() * (xhat * wdz).abs().mean(-1, keepdim=True) + wdz.abs().mean(-1, keepdim=True))
    if dx is not None:
        dxs, t = dxs + dx.to(dtype), t + dx.to(dtype).abs()
    inv_keep = 1.0 / (1.0 - p)
    s0 = keep0.to(dtype) * inv_keep if p > 0.0 else torch.ones_like(dxs)  # d x / d (x0 * rowscale * colscale)
    if rowscale is not None:
        s0 = s0 * rowscale.to(dtype)[:, None]
    out = dict(dresidual=dxs, t=t, dx1=None, t_dx1=None, dcolscale=None, t_dcolscale=None, dw1=None, db1=None, t_dw1=None,
               t_db1=None)
    if colscale is not None:
        out["dcolscale"] = (dxs * s0 * x0.to(dtype)).sum(0)
        out["t_dcolscale"] = (t * (s0 * x0.to(dtype)).abs()).sum(0)
        s0 = s0 * colscale.to(dtype)
    out["dx0"], out["t_dx0"] = dxs * s0, t * s0.abs()
    if has_x1:
        s1 = keep1.to(dtype) * inv_keep if p > 0.0 else torch.ones_like(dxs)
        out["dx1"], out["t_dx1"] = dxs * s1, t * s1.abs()
    for i, dz in (("0", dz0),) + ((("1", dz1),) if w1 is not None else ()):
        dz = dz.to(dtype)
        out["dw" + i], out["db" + i] = (dz * xhat).sum(0), dz.sum(0)
        out["t_dw" + i], out["t_db" + i] = (dz * xhat).abs().sum(0), dz.abs().sum(0)
    return out
