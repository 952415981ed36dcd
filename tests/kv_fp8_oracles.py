"""Oracle of the fp8 KV-cache format, independent of pyrecover_amd.ops.reference and of torch's float8 cast:
the rule in fp64 / integers with an explicit OCP e4m3fn table.

A cache row x (D values) is stored as D e4m3fn bytes and one fp32 scale 2^e:
  amax = max |x_i|; amax == 0: e = 0 (scale 1), every byte 0x00 (also for -0.0); otherwise (m, k) = frexp(amax), m in [0.5, 1),
  e = clamp(k - 9 + (m > 0.875), -126, 127), the smallest e with amax * 2^-e <= 448 = 0.875 * 2^9;
  byte_i = e4m3fn_rne(x_i * 2^-e); the dequantized value is byte_i * 2^e.
Inputs are taken as fp32 (16-bit values convert exactly); every product here is exact in fp64.

e4m3fn: 1 sign, 4 exponent (bias 7), 3 mantissa bits; exponent 0 is subnormal (m / 8 * 2^-6); 0x7F / 0xFF are
NaN, there is no infinity, and the largest finite value is 0x7E = 448.

``defect`` seeds one mistake a kernel could make (tests/test_kv_fp8.py shows the comparison catches each):
  truncate     round toward zero instead of to nearest even
  e_plus_one   e one too large (half the resolution)      e_minus_one  e one too small (saturates at 448)
  token_scale  one amax for the whole token (all kv heads) instead of one per head row
"""
import functools

import numpy as np
import torch

DEFECTS = ("truncate", "e_plus_one", "e_minus_one", "token_scale")


def _decode_table():
    t = np.empty(256, dtype=np.float64)
    for b in range(256):
        exp, man = (b >> 3) & 15, b & 7
        if exp == 15 and man == 7:
            v = float("nan")
        elif exp == 0:
            v = man / 8.0 * 2.0 ** -6
        else:
            v = (1.0 + man / 8.0) * 2.0 ** (exp - 7)
        t[b] = -v if b & 0x80 else v
    return t


DECODE = _decode_table()
POSITIVE = DECODE[:0x7F]  # codes 0x00 .. 0x7E: 0 .. 448, ascending
assert POSITIVE[-1] == 448.0 and bool((np.diff(POSITIVE) > 0).all())


def e4m3_encode(y: np.ndarray, truncate: bool = False) -> np.ndarray:
    """fp64 values -> e4m3fn codes, round to nearest even (ties to the even code); magnitudes above 448
    saturate at 448 (the rule never produces one), NaN gives 0x7F; the sign of zero is kept."""
    a = np.abs(y)
    nan = np.isnan(a)
    a = np.minimum(np.where(nan, 0.0, a), 448.0)
    hi = np.searchsorted(POSITIVE, a, side="left")  # first code whose value is >= a
    lo = np.maximum(hi - 1, 0)
    d_hi, d_lo = POSITIVE[hi] - a, a - POSITIVE[lo]  # exact: dyadic values a few binades apart
    if truncate:
        code = np.where(d_hi == 0, hi, lo)
    else:
        code = np.where(d_hi < d_lo, hi, np.where(d_lo < d_hi, lo, np.where(hi % 2 == 0, hi, lo)))
    code = code.astype(np.uint8) | (np.signbit(y).astype(np.uint8) << 7)
    return np.where(nan, np.uint8(0x7F), code).astype(np.uint8)


def scale_exponent(amax: np.ndarray) -> np.ndarray:
    m, k = np.frexp(amax)
    e = np.clip(k.astype(np.int64) - 9 + (m > 0.875), -126, 127)
    return np.where(amax == 0, 0, e)


def quantize(x: torch.Tensor, defect=None):
    """x [..., D] (for ``token_scale``: [..., Hkv, D]) -> (bytes uint8 [..., D], scale fp32 [...])."""
    assert defect is None or defect in DEFECTS
    x64 = x.detach().cpu().float().double().numpy()
    amax = np.abs(x64).max(axis=-1)
    if defect == "token_scale":
        amax = np.broadcast_to(amax.max(axis=-1, keepdims=True), amax.shape)
    e = scale_exponent(amax)
    if defect == "e_plus_one":
        e = e + 1
    elif defect == "e_minus_one":
        e = e - 1
    y = np.ldexp(x64, -e[..., None])
    q = e4m3_encode(y, truncate=defect == "truncate")
    q = np.where((amax == 0)[..., None], np.uint8(0), q)  # an all-zero row is all bytes 0, whatever the signs
    scale = np.ldexp(np.float64(1.0), e).astype(np.float32)
    return torch.from_numpy(np.ascontiguousarray(q)), torch.from_numpy(np.ascontiguousarray(scale))


def dequantize(q: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """bytes [..., D], scale [...] -> fp64 values byte_i * scale (exact)."""
    v = DECODE[q.detach().cpu().numpy()] * scale.detach().cpu().double().numpy()[..., None]
    return torch.from_numpy(v)


def edge_rows(dtype, D: int) -> torch.Tensor:
    """[n, D] rows of ``dtype`` (bf16 / fp16) at the corners of the rule: all zero; amax exactly
    448 * 2^j and the next value of the dtype above it (the m > 0.875 boundary) for a few j; amax the
    dtype's largest finite value; amax 2^-130 (bf16 only: the clamp of e at -126); mixed signs with -0.0."""
    g = torch.Generator().manual_seed(1234)
    fi = torch.finfo(dtype)
    rows = [torch.zeros(D)]

    def filled(top, sign=1.0):
        r = (torch.rand(D, generator=g) * 2 - 1) * top * 0.9
        r[int(torch.randint(0, D, (1,), generator=g))] = sign * top
        return r

    js = (-9, -3, 0, 4) if dtype == torch.float16 else (-40, -9, 0, 4, 60)
    for j in js:
        top = 448.0 * 2.0 ** j
        above = torch.nextafter(torch.tensor(top, dtype=dtype), torch.tensor(float("inf"), dtype=dtype)).item()
        rows += [filled(top), filled(top, -1.0), filled(above)]
    rows.append(filled(fi.max))
    if dtype == torch.bfloat16:
        tiny = torch.zeros(D)
        tiny[3], tiny[5], tiny[6] = 2.0 ** -130, -(2.0 ** -131), 2.0 ** -133
        rows.append(tiny)
    mixed = filled(3.0)
    mixed[::2] = -mixed[::2].abs()
    mixed[1], mixed[2] = -0.0, 0.0
    rows.append(mixed)
    neg_zero = torch.zeros(D)
    neg_zero[::3] = -0.0
    rows.append(neg_zero)
    out = torch.stack(rows).to(dtype)
    assert bool(torch.isfinite(out.float()).all())
    return out


RECIPES = ("peaked", "all_negative", "all_large", "stair5", "stair9")
GROUPS = ((2, 2), (4, 2), (4, 1), (8, 1))  # (Hq, Hkv): GQA groups of 1, 2, 4, 8 -- every head-tile arm of the kernel


@functools.lru_cache(maxsize=None)
def decode_case(name, D, dtype, Hq, Hkv, KC=256):
    """``_decode_case`` of tests/test_attention_rowerr_gpu.py over an fp8 cache: one ragged batch with lengths
    1, KC - 1, KC, KC + 1, 3 KC + 17 and cap = max + 7. The recipe's K and V are quantized by the oracle
    (c.kq, c.ks, c.vq, c.vs); the fp64 oracle, the error scale and the lse bound are computed on the
    dequantized values (c.k, c.v: exact in ``dtype``)."""
    from tests import attention_oracles as A

    lens = (1, KC - 1, KC, KC + 1, 3 * KC + 17)
    B, cap = len(lens), max(lens) + 7
    q, k, v, _, scale = A.recipe(name, B, cap, Hq, Hkv, D, dtype, causal=False)
    c = A.Case()
    c.name, c.shape, c.dtype, c.causal, c.scale = name, (B, cap, Hq, Hkv, D), dtype, False, scale
    c.kq, c.ks = quantize(k)
    c.vq, c.vs = quantize(v)
    k64, v64 = dequantize(c.kq, c.ks), dequantize(c.vq, c.vs)
    c.k, c.v = k64.to(dtype), v64.to(dtype)
    assert torch.equal(c.k.double(), k64) and torch.equal(c.v.double(), v64)
    c.q = q[:, :1].contiguous()
    c.kv_len = torch.tensor(lens, dtype=torch.int32)
    c.vis = A.visibility(B, 1, cap, False, kv_len=c.kv_len)
    c.o, c.lse = A.forward_oracle(c.q, c.k, c.v, scale, c.vis)
    (c.m_o,) = A.abs_oracle(c.q, c.k, c.v, None, c.lse, None, scale, c.vis, dtype)
    c.lse_bound, c.smax = A.lse_bound(c.q, c.k, scale, c.vis, c.lse)
    return c


def random_rows(dtype, n: int, D: int, binades: int = 40, seed: int = 0) -> torch.Tensor:
    """[n, D] normal rows, row r scaled by 2^(r mod binades - binades / 2) (kept inside the dtype's range)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, D, generator=g)
    ex = (torch.arange(n) % binades) - binades // 2
    if dtype == torch.float16:
        ex = ex.clamp(-12, 12)
    return (x * torch.ldexp(torch.ones(n), ex)[:, None]).to(dtype)
