"""Stateless stochastic rounding of fp32 values to bf16 / fp16 (``--stochastic-rounding``).

The same rule as ``csrc/kernels/philox_sr.h``, written in torch integer ops: the tests' oracle for the
HIP kernels and the path CPU (and gloo) runs take, on any device.

An element's 16 random bits are a pure function of ``(seed, t, idx, stream)``: ``idx`` is its int64
position in the flat parameter buffer, ``t`` the AdamW step number its bias corrections use
(1-based; applied steps under ``--loss-scale``), ``stream`` the tensor (0 parameters, 1 exp_avg,
2 exp_avg_sq). With ``g = idx >> 3`` and ``lane = idx & 7``::

    out  = philox4x32_10(counter=(g & 0xffffffff, g >> 32, t, stream), key=(seed & 0xffffffff, seed >> 32))
    r    = (out[lane >> 1] >> (16 * (lane & 1))) & 0xffff

Rounding fp32 ``x`` to the 16-bit type T: non-finite values and ``|x|`` above T's largest finite value
take the plain round-to-nearest cast. Otherwise ``lo`` is ``x`` truncated toward zero to T, ``hi`` the
next T value away from zero, ``tfrac = floor((|x| - |lo|) / (|hi| - |lo|) * 65536)``, and the result is
``hi`` when ``r < tfrac``, else ``lo``. The sign is kept (-0 stays -0). For bf16 that is
``(bits >> 16) + (r < (bits & 0xffff))``. The expectation differs from ``x`` by less than 2^-16 ulp.
"""
from __future__ import annotations

import torch

STREAM_P, STREAM_M, STREAM_V = 0, 1, 2
MODES = {"params": 1, "all": 7}  # --stochastic-rounding mode -> tensor mask (bit 0 p, 1 exp_avg, 2 exp_avg_sq)

_M0, _M1 = 0xD2511F53, 0xCD9E8D57
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LOW = 0xFFFFFFFF


def _mulhilo(a: int, b: torch.Tensor):
    """32 x 32 -> (hi, lo) of constant ``a`` and int64 tensor ``b`` holding uint32 values, without
    overflowing int64: b is split into 16-bit halves."""
    t0 = a * (b & 0xFFFF)  # < 2^48
    t1 = a * (b >> 16)  # < 2^48; the product is t0 + (t1 << 16)
    lo = (t0 + ((t1 & 0xFFFF) << 16)) & _LOW
    hi = ((t1 >> 16) + ((t0 + ((t1 & 0xFFFF) << 16)) >> 32)) & _LOW
    return hi, lo


def philox4x32_10(counter, key):
    """Philox4x32-10. ``counter``: four int64 tensors (or ints) holding uint32 values, ``key``: two
    Python ints. Returns the four output words as int64 tensors holding uint32 values."""
    c = [torch.as_tensor(x, dtype=torch.int64) for x in counter]
    dev = next((x.device for x in c if x.dim()), c[0].device)
    c0, c1, c2, c3 = torch.broadcast_tensors(*[x.to(dev) & _LOW for x in c])
    k0, k1 = int(key[0]) & _LOW, int(key[1]) & _LOW
    for _ in range(10):
        hi0, lo0 = _mulhilo(_M0, c0)
        hi1, lo1 = _mulhilo(_M1, c2)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + _W0) & _LOW, (k1 + _W1) & _LOW
    return c0, c1, c2, c3


def random16(idx: torch.Tensor, t: int, stream: int, seed: int) -> torch.Tensor:
    """The 16 random bits (int64 tensor, values 0..65535) of the elements at flat positions ``idx``."""
    idx = torch.as_tensor(idx, dtype=torch.int64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    g, lane = idx >> 3, idx & 7
    out = philox4x32_10((g & _LOW, (g >> 32) & _LOW, int(t), int(stream)), (seed & _LOW, seed >> 32))
    word = torch.stack(out, dim=-1).gather(-1, (lane >> 1).unsqueeze(-1)).squeeze(-1)
    return (word >> (16 * (lane & 1))) & 0xFFFF


def stochastic_round(x: torch.Tensor, dtype: torch.dtype, idx: torch.Tensor, t: int, stream: int, seed: int) -> torch.Tensor:
    """fp32 ``x`` -> ``dtype`` (bf16 or fp16), element i rounded with the bits of flat position ``idx[i]``."""
    if x.dtype != torch.float32:
        raise ValueError(f"stochastic_round expects fp32 values, got {x.dtype}")
    if dtype not in (torch.bfloat16, torch.float16):
        raise ValueError(f"stochastic_round rounds to bf16 or fp16, not {dtype}")
    x = x.contiguous()
    r = random16(torch.as_tensor(idx, dtype=torch.int64).to(x.device), t, stream, seed).reshape(x.shape)
    plain = x.to(dtype)
    if dtype == torch.bfloat16:
        bits = x.view(torch.int32).to(torch.int64) & _LOW
        out16 = (bits >> 16) + (r < (bits & 0xFFFF)).to(torch.int64)
        out16 = torch.where(out16 >= 0x8000, out16 - 0x10000, out16).to(torch.int16)
        use_plain = (bits & 0x7FFFFFFF) > 0x7F7F0000  # NaN, inf, above bf16's largest finite value
        return torch.where(use_plain, plain, out16.view(torch.bfloat16))
    # fp16, the general rule in exact fp64 arithmetic: u = |hi| - |lo| is 2^(e - 10) in the binade
    # 2^e <= |x| < 2^(e + 1) and 2^-24 below 2^-14 (subnormal results)
    xd = x.double()
    ax = xd.abs()
    _, ex = torch.frexp(ax)  # ax = m * 2^ex, m in [0.5, 1)
    e = (ex.to(torch.int64) - 1).clamp(min=-14, max=15)
    u = torch.ldexp(torch.ones_like(ax), e - 10)
    q = ax / u  # exact: u is a power of two
    lo = q.floor()
    tfrac = ((q - lo) * 65536.0).floor().to(torch.int64)
    n = lo + (r < tfrac).to(torch.float64)
    sr = torch.copysign(n * u, xd).to(dtype)  # n * u is an fp16 value: this cast is exact
    use_plain = ~torch.isfinite(x) | (ax > 65504.0)
    return torch.where(use_plain, plain, sr)
