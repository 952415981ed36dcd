"""Oracle of the MXFP4 KV-cache format (csrc/kernels/attention_decode_fp4.hip states the rule), independent of
pyrecover_amd.ops.reference: the scale rule on the fp32 bits in integers, the code by a nearest search in the table
of the 8 e2m1 magnitudes (ties to the even code) on |x| * 2^-e, exact in fp64."""
import functools

import numpy as np
import torch

MAGNITUDES = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
VALUES = np.concatenate([MAGNITUDES, -MAGNITUDES])  # the 16 nibble values


def scale_exponent(amax32: np.ndarray) -> np.ndarray:
    bits = amax32.astype(np.float32).view(np.uint32).astype(np.int64)
    E, frac = bits >> 23, bits & 0x7FFFFF
    e = np.clip(E - 126 - 3 + (frac > 0x400000), -127, 127)  # normal: k = E - 126, m > 0.75 <=> frac > 1/2
    e = np.where(E == 0, -127, e)  # subnormal: k <= -126, below the clamp
    return np.where(bits == 0, 0, e)


def quantize(x: torch.Tensor):
    x32 = x.detach().cpu().float().numpy()
    blk = x32.reshape(*x32.shape[:-1], -1, 32)
    amax = np.abs(blk).max(axis=-1)
    e = scale_exponent(amax)
    y = np.ldexp(np.abs(blk).astype(np.float64), -e[..., None])
    assert float(y.max(initial=0.0)) <= 6.0  # nothing saturates
    hi = np.searchsorted(MAGNITUDES, y, side="left")  # first code whose magnitude is >= y
    lo = np.maximum(hi - 1, 0)
    d_hi, d_lo = MAGNITUDES[hi] - y, y - MAGNITUDES[lo]
    code = np.where(d_hi < d_lo, hi, np.where(d_lo < d_hi, lo, np.where(hi % 2 == 0, hi, lo)))
    nib = (code | np.signbit(blk).astype(np.int64) << 3) * (amax != 0)[..., None]
    nib = nib.reshape(*x32.shape[:-1], -1, 2).astype(np.uint8)
    return torch.from_numpy(nib[..., 0] | nib[..., 1] << 4), torch.from_numpy((e + 127).astype(np.uint8))


def dequantize(q: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    b = q.detach().cpu().numpy()
    v = VALUES[np.stack([b & 15, b >> 4], axis=-1).reshape(*b.shape[:-1], -1, 32)]
    e = scale.detach().cpu().numpy().astype(np.int64) - 127
    return torch.from_numpy(np.ldexp(v, e[..., None]).reshape(*b.shape[:-1], -1))


def edge_rows(dtype, D: int) -> torch.Tensor:
    """[n, D] rows of ``dtype`` at the corners of the rule: an all-zero block beside a large one, a single non-zero
    element, amax exactly 6 * 2^j and the dtype's next value above it, every tie (both signs), -0.0 in zero and
    non-zero blocks, 16-bit subnormals, the largest finite value."""
    g = torch.Generator().manual_seed(4321)
    fi, inf = torch.finfo(dtype), torch.tensor(float("inf"), dtype=dtype)
    rows = torch.zeros(3, D)  # all zero; zero block beside a large one; a single element
    rows[1, 32:], rows[2, 37] = torch.randn(D - 32, generator=g) * 1000, -0.3
    rows = list(rows)
    for j in ((-9, 0, 4) if dtype == torch.float16 else (-100, -9, 0, 4, 100)):
        top = 6.0 * 2.0 ** j
        for amax in (top, torch.nextafter(torch.tensor(top, dtype=dtype), inf).item()):
            r = (torch.rand(D, generator=g) * 2 - 1) * top
            r[5], r[40] = amax, -amax
            rows.append(r)
        ties = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 6.0]) * 2.0 ** j
        rows.append(torch.cat([ties, -ties, torch.zeros(D - 16)]))
    sub, neg0, top = torch.zeros(D), torch.zeros(D), torch.randn(D, generator=g) * (fi.max / 8)
    sub[3], sub[5], sub[6], sub[40] = fi.smallest_normal / 4, -fi.smallest_normal / 8, fi.smallest_normal, fi.smallest_normal / 2
    neg0[::3], neg0[33], top[0] = -0.0, 1.0, fi.max
    return torch.stack(rows + [sub, neg0, top]).to(dtype)


@functools.lru_cache(maxsize=None)
def decode_case(name, D, dtype, Hq, Hkv, KC=256):
    """``decode_case`` of tests/kv_fp8_oracles.py with this module's quantize / dequantize in place of its own."""
    from unittest import mock

    from tests import kv_fp8_oracles as Q8

    with mock.patch.multiple(Q8, quantize=quantize, dequantize=dequantize):
        return Q8.decode_case.__wrapped__(name, D, dtype, Hq, Hkv, KC)
