"""fp64 oracles, same-dtype baselines, input recipes and error bounds for the kernel edge tests.

Shared by tests/test_kernel_edges_gpu.py (HIP kernels against these oracles, on the GPU) and
tests/test_kernel_oracles.py (the baselines alone against the same caps, on the CPU), so an input
recipe is validated before a kernel ever sees it. Everything here is device-agnostic torch.

Oracle of an op: fp64 math on the upcast inputs with only the rounding points the kernel documents
(h = round(x + delta); RMSNorm rounds the normalized value before the weight multiply; SwiGLU rounds
silu(g) and dy*u; one final rounding to the storage dtype). Outputs are returned as fp64 tensors that
hold storage-dtype values; statistics the kernels keep in fp32 (rstd, mean, lse, loss) stay unrounded.
Baseline of an op: the project's own same-dtype PyTorch reference (pyrecover_amd/ops/reference.py, or
the CPU branch of ops/fused.py where reference.py has none), fp32 opmath.

Bounds:
  16-bit storage  max|kernel - oracle| <= 2 * max|baseline - oracle| + 1 ulp(storage) at max|oracle|
                  (both sides do fp32 math and one final rounding; the factor 2 and the ulp cover an
                  intermediate that lands on the other side of a tie)
  fp32 storage    max|kernel - oracle| <= min(4 * measured, 2^-16) * max|oracle|, `measured` being the
                  kernel's relative error recorded in the GPU test module; the 2^-16 cap is a condition,
                  not a measurement: an fp32 path that goes through 16-bit storage errs by >= 2^-12.
"""
import math

import torch
import torch.nn.functional as F

from pyrecover_amd.ops import reference as R

DTYPES = (torch.bfloat16, torch.float16, torch.float32)
MANT_BITS = {torch.bfloat16: 7, torch.float16: 10, torch.float32: 23}
FP32_CAP = 2.0 ** -16
EPS = 1e-5

NORM_SHAPES = [(1, 8), (3, 520), (15, 512), (16, 1032), (1025, 2048), (2051, 2056), (5, 4104), (4, 8192)]
XENT_SHAPES = [(5, 8, 8), (7, 1001, 1008), (4, 2047, 2048), (4, 2049, 2056), (2, 50257, 50264)]  # T, V, row stride
ROPE_SHAPES = [(4096, 512, 10 * 128, 128), (64, 16, 128, 64), (6, 3, 16, 8)]  # tokens, S, ncols, head_dim
ROPE_MAX_OFFSET = 64
SWIGLU_SHAPE = (2050, 2056)  # T, F
EMBED_SHAPES = [(1000, 8, 5), (50, 520, 4099), (1000, 4096, 1027), (16, 1024, 4096)]  # V, D, tokens
GRAD_NORM_SIZES = [1, 7, 8, 9, 2055, (1 << 21) + 3]
GRAD_NORM_PRE_SCALE = 0.5


def dname(dtype) -> str:
    return str(dtype).replace("torch.", "")


def ulp_at(dtype, mag: float) -> float:
    """Spacing of `dtype` at magnitude `mag`."""
    if mag <= 0.0:
        return 0.0
    return 2.0 ** (math.floor(math.log2(mag)) - MANT_BITS[dtype])


def rt(x64: torch.Tensor, dtype) -> torch.Tensor:
    """One rounding to the storage dtype, kept as fp64."""
    return x64.to(dtype).double()


def err(a: torch.Tensor, oracle: torch.Tensor) -> float:
    return (a.double() - oracle).abs().max().item()


def approx_bound(dtype, base: torch.Tensor, oracle: torch.Tensor) -> float:
    return 2.0 * err(base, oracle) + ulp_at(dtype, oracle.abs().max().item())


def fp32_bound(measured_rel: float, oracle: torch.Tensor) -> float:
    return min(4.0 * measured_rel, FP32_CAP) * oracle.abs().max().item()


def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def _to(device, dtype, *ts):
    return [t.to(dtype).to(device) for t in ts]


# ------------------------------------------------------------------------------------------------
# RMSNorm / LayerNorm
def norm_inputs(rows, D, dtype, device, layernorm=False):
    """x, delta, w, b, dy, dres, dwb0 (a non-zero [2D] gradient to accumulate onto; RMSNorm uses [:D])."""
    g = _gen(rows * 10007 + D + (1 if layernorm else 0))
    x = torch.randn(rows, D, generator=g) + (0.5 if layernorm else 0.0)
    delta = torch.randn(rows, D, generator=g)
    w = 1 + 0.1 * torch.randn(D, generator=g)
    b = 0.1 * torch.randn(D, generator=g)
    dy = torch.randn(rows, D, generator=g)
    dres = torch.randn(rows, D, generator=g)
    dwb0 = torch.randn(2 * D, generator=g)
    return _to(device, dtype, x, delta, w, b, dy, dres, dwb0)


def _h(x, delta):
    return x.double() if delta is None else rt(x.double() + delta.double(), x.dtype)


def rmsnorm_fwd_oracle(x, delta, w, eps=EPS):
    h = _h(x, delta)
    rstd = torch.rsqrt(h.pow(2).mean(-1) + eps)
    nb = rt(h * rstd[:, None], x.dtype)
    return h, rt(nb * w.double(), x.dtype), rstd


def rmsnorm_bwd_oracle(dy, h, w, rstd, dres, dw0):
    dt, D = h.dtype, h.shape[-1]
    h64, dy64, r = h.double(), dy.double(), rstd.double()[:, None]
    nb = rt(h64 * r, dt)
    g = rt(dy64 * w.double(), dt)
    dot = (g * h64).sum(-1, keepdim=True)
    dx = rt(r * (g - h64 * (r * r * dot / D)), dt)
    if dres is not None:
        dx = rt(dx + dres.double(), dt)
    dw = (dy64 * nb).sum(0)
    if dw0 is not None:
        dw = dw + dw0.double()
    return dx, rt(dw, dt)


def rmsnorm_fwd_base(x, delta, w, eps=EPS):
    return R.rmsnorm_fwd(x, delta, w, eps)


def rmsnorm_bwd_base(dy, h, w, rstd, dres, dw0):
    dx, dw = R.rmsnorm_bwd(dy, h, w, rstd, dres)
    dw = dw.to(h.dtype)
    return dx, dw if dw0 is None else dw0 + dw  # as ops/fused.py accumulates on the reference path


def layernorm_fwd_oracle(x, delta, w, b, eps=EPS):
    h = _h(x, delta)
    mean = h.mean(-1)
    rstd = torch.rsqrt((h - mean[:, None]).pow(2).mean(-1) + eps)
    y = rt((h - mean[:, None]) * rstd[:, None] * w.double() + b.double(), x.dtype)
    return h, y, mean, rstd


def layernorm_bwd_oracle(dy, h, w, mean, rstd, dres, dwb0):
    dt = h.dtype
    dy64, r = dy.double(), rstd.double()[:, None]
    xh = (h.double() - mean.double()[:, None]) * r
    g = dy64 * w.double()
    s1 = g.mean(-1, keepdim=True)
    s2 = (g * xh).mean(-1, keepdim=True)
    dx = rt(r * (g - s1 - xh * s2), dt)
    if dres is not None:
        dx = rt(dx + dres.double(), dt)
    dwb = torch.cat([(dy64 * xh).sum(0), dy64.sum(0)])
    if dwb0 is not None:
        dwb = dwb + dwb0.double()
    return dx, rt(dwb, dt)


def layernorm_fwd_base(x, delta, w, b, eps=EPS):
    """ops/fused.py's reference branch; mean and rstd in fp32 opmath."""
    h = x if delta is None else x + delta
    y = F.layer_norm(h, (h.shape[-1],), w, b, eps)
    hf = R.up(h)
    mean = hf.mean(-1)
    rstd = torch.rsqrt((hf - mean[:, None]).pow(2).mean(-1) + eps)
    return h, y, mean, rstd


def layernorm_bwd_base(dy, h, w, b, dres, dwb0, eps=EPS):
    with torch.enable_grad():
        hh, ww, bb = (t.detach().requires_grad_() for t in (h, w, b))
        yy = F.layer_norm(hh, (h.shape[-1],), ww, bb, eps)
        gx, gw, gb = torch.autograd.grad(yy, (hh, ww, bb), dy)
    dx = gx if dres is None else gx + dres
    dwb = torch.cat([gw.reshape(-1), gb.reshape(-1)]).to(h.dtype)
    return dx, dwb if dwb0 is None else dwb0 + dwb


# ------------------------------------------------------------------------------------------------
# Cross-entropy
IGNORE = -100


def xent_inputs(T, V, ld, dtype, device):
    """logits = [:, :V] view of a [T, ld] buffer whose padding columns hold the largest finite value;
    row 0 spreads over +-80, row 1 has a single dominant logit, the rest are 3 * randn. Labels hold 0,
    V - 1 (inside the scalar tail when V % 8 != 0) and, from three rows on, ignore_index."""
    g = _gen(T * 100003 + V)
    x = 3 * torch.randn(T, V, generator=g)
    x[0] = torch.linspace(-80, 80, V)[torch.randperm(V, generator=g)]
    x[1] = torch.randn(V, generator=g)
    x[1, min(3, V - 2)] = 30.0
    buf = torch.full((T, ld), torch.finfo(dtype).max, dtype=dtype)
    buf[:, :V] = x.to(dtype)
    labels = torch.randint(0, V, (T,), generator=g)
    labels[0] = 0
    labels[1] = V - 1
    if T > 2:
        labels[2] = IGNORE
    buf = buf.to(device)
    return buf, buf[:, :V], labels.to(device)


def xent_oracle(logits, labels, gscale, ignore_index=IGNORE):
    """lse [T], mean loss, n_valid, dlogits (storage-dtype values) for d loss = gscale."""
    x = logits.double()
    T = x.shape[0]
    lse = torch.logsumexp(x, dim=-1)
    valid = labels.ne(ignore_index)
    n = valid.sum()
    safe = labels.clamp(0, x.shape[1] - 1)
    loss_row = torch.where(valid, lse - x.gather(1, safe[:, None])[:, 0], torch.zeros_like(lse))
    p = torch.exp(x - lse[:, None])
    p[torch.arange(T, device=x.device), safe] -= valid.double()
    d = p * valid.double()[:, None] * (gscale / n.double())
    return lse, loss_row.sum() / n, int(n.item()), rt(d, logits.dtype)


def xent_base(logits, labels, gscale, ignore_index=IGNORE):
    with torch.enable_grad():
        lf = R.up(logits).detach().clone().requires_grad_()
        loss = R.cross_entropy_ref(lf, labels, ignore_index)
        loss.backward()
    return torch.logsumexp(R.up(logits), dim=-1), loss.detach(), (gscale * lf.grad).to(logits.dtype)


# ------------------------------------------------------------------------------------------------
# RoPE
def rope_inputs(ntok, S, ncols, D, dtype, device):
    """buf [ntok, 8 + ncols + 2 * D]; x = buf[:, 8:] so that guard columns lie on both sides of the rotated
    ones; fp32 table for S + ROPE_MAX_OFFSET positions."""
    g = _gen(ntok + ncols + D)
    buf = torch.randn(ntok, 8 + ncols + 2 * D, generator=g).to(dtype).to(device)
    tab = R.rope_table(R.precompute_freqs_cis(D, S + ROPE_MAX_OFFSET, 10000.0)).to(device)
    return buf, tab


def rope_oracle(x2d, ncols, tab, D, S, pos_offset, inverse):
    T = x2d.shape[0]
    v = x2d[:, :ncols].double().reshape(T, ncols // D, D // 2, 2)
    pos = torch.arange(T, device=x2d.device) % S + pos_offset
    cs = tab[pos].double()  # [T, D/2, 2]
    c, s = cs[..., 0][:, None], cs[..., 1][:, None] * (-1.0 if inverse else 1.0)
    a, b = v[..., 0], v[..., 1]
    return rt(torch.stack([a * c - b * s, a * s + b * c], dim=-1).reshape(T, ncols), x2d.dtype)


def rope_base(x2d, ncols, tab, D, S, pos_offset, inverse):
    xb = x2d.clone()
    R.rope_inplace_2d(xb, ncols, tab[pos_offset:], D, S, inverse=inverse)
    return xb[:, :ncols]


# ------------------------------------------------------------------------------------------------
# SwiGLU
def swiglu_inputs(T, Fdim, dtype, device):
    """gu = [:, 8:8+2F] view of a wider buffer, dy likewise, plus a second wide buffer for the output."""
    g = _gen(T + Fdim)
    gbuf = torch.randn(T, 2 * Fdim + 16, generator=g).to(dtype).to(device)
    dbuf = torch.randn(T, Fdim + 16, generator=g).to(dtype).to(device)
    obuf = torch.randn(T, 2 * Fdim + 16, generator=g).to(dtype).to(device)
    return gbuf, dbuf, obuf


def swiglu_fwd_oracle(g, u):
    a = rt(g.double() * torch.sigmoid(g.double()), g.dtype)
    return rt(a * u.double(), g.dtype)


def swiglu_bwd_oracle(dy, g, u):
    dt = g.dtype
    g64, u64, d64 = g.double(), u.double(), dy.double()
    sg = torch.sigmoid(g64)
    a = rt(g64 * sg, dt)
    da = rt(d64 * u64, dt)
    return rt(da * sg * (1 + g64 * (1 - sg)), dt), rt(d64 * a, dt)


# ------------------------------------------------------------------------------------------------
# Embedding
def embed_inputs(V, D, ntok, dtype, device):
    """W, ids, dout, dW0. dout and dW0 are multiples of 1/8 (|dout| <= 1, |dW0| <= 4), so every partial
    sum of up to 2^17 rows is a multiple of 1/8 below 2^21: exact in fp32 in any order."""
    g = _gen(V + D + ntok)
    W = torch.randn(V, D, generator=g)
    if V == 16:
        ids = torch.full((ntok,), 5, dtype=torch.long)  # one id for every token
    else:
        ids = torch.randint(0, V, (ntok,), generator=g)
        ids[ids == 3] = 0  # rows 3 and V - 4 stay untouched at every size; rows 0 and V - 1 are used
        ids[ids == V - 4] = V - 1
    dout = torch.randint(-8, 9, (ntok, D), generator=g) / 8.0
    dW0 = torch.randint(-32, 33, (V, D), generator=g) / 8.0
    W, dout, dW0 = _to(device, dtype, W, dout, dW0)
    return W, ids.to(device), dout, dW0


def embed_bwd_oracle(ids, dout, V, dW0):
    keep = (ids >= 0) & (ids < V)
    acc = torch.zeros(V, dout.shape[-1], dtype=torch.float64, device=dout.device)
    acc.index_add_(0, ids[keep], dout.double()[keep])
    if dW0 is not None:
        acc = acc + dW0.double()
    return rt(acc, dout.dtype)


# ------------------------------------------------------------------------------------------------
# grad_norm
def grad_norm_input(n, dtype, device):
    return torch.randn(n, generator=_gen(n)).to(dtype).to(device)


def grad_norm_oracle(x, pre_scale=GRAD_NORM_PRE_SCALE) -> float:
    return x.double().norm().item() * pre_scale


def grad_norm_base(x, pre_scale=GRAD_NORM_PRE_SCALE) -> float:
    return x.float().norm().item() * pre_scale
