"""Oracles for the stateless sampler (csrc/kernels/sample.hip, ops/reference.py::sample_philox_ref).

Not a test file. It holds the sampling rule in fp64 (stable sort, cumsum), the Philox uniform in plain
Python integers, the acceptance check the sampling tests share, seeded defects that keep the check
honest, and the input recipes.

The rule, for one row of logits x, temperature T > 0, top_k (0: off), top_p in (0, 1] and a uniform u:
tokens are ranked by z = x / T descending, ties by ascending id, under NaN < -inf < finite < +inf; top-k
keeps every token with z >= the k-th largest z; top-p keeps the shortest prefix of the ranking whose
softmax mass over the top-k survivors reaches top_p (dropped iff the mass ranked above is >= top_p, the
first always stays); the draw is the first kept token whose cumulative renormalised mass exceeds u. A row
whose maximum is not finite, and T == 0, give the lowest id holding the maximum.

Acceptance. A 16-bit kernel sums fp32 masses in another order than this file does, so where u falls
within rounding of a boundary two neighbouring tokens are both right. Token t is accepted for
(x, u, T, k, p) when, for some nucleus among top_p, top_p - DELTA and top_p + DELTA, t is kept and its
fp64 CDF interval, widened by DELTA on both sides, contains u. DELTA = 2^-14 of the total mass covers the
fp32 exp2 error (an argument of magnitude up to ~150 carries 2^-24 relative error: about 2^-17 of a
bin's mass) and a 65,536-term fixed-order fp32 sum (about 2^-16) with margin. When u is farther than
DELTA from every boundary exactly one token is acceptable and the check is exact; ``near_boundary`` says
which rows are not in that position.
"""
from __future__ import annotations

import torch

DELTA = 2.0 ** -14
SAMPLE_STREAM = 3

_M0, _M1, _W0, _W1, _LOW = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF


def philox4x32_10_int(counter, key):
    """Philox4x32-10 on Python ints (Salmon et al., SC'11): counter 4 words, key 2 words -> 4 words."""
    c0, c1, c2, c3 = [int(c) & _LOW for c in counter]
    k0, k1 = int(key[0]) & _LOW, int(key[1]) & _LOW
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & _LOW, p1 & _LOW, ((p0 >> 32) ^ c3 ^ k1) & _LOW, p0 & _LOW
        k0, k1 = (k0 + _W0) & _LOW, (k1 + _W1) & _LOW
    return c0, c1, c2, c3


def uniform(pos, seed: int) -> torch.Tensor:
    """fp64 [B]: row b's uniform at absolute position pos[b]. (out[0] >> 8) * 2^-24 is exact in fp32."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    key = (seed & _LOW, seed >> 32)
    return torch.tensor([(philox4x32_10_int((b, int(p), 0, SAMPLE_STREAM), key)[0] >> 8) * 2.0 ** -24
                         for b, p in enumerate(torch.as_tensor(pos).reshape(-1).tolist())], dtype=torch.float64)


class Ranking:
    """The fp64 rule for the rows of one logits tensor [B, V]. The stable sort does not depend on T > 0
    and is done once; every (T, k, p) setting reuses it. Computes on ``device`` (default: the CPU)."""

    def __init__(self, x: torch.Tensor, device="cpu"):
        x = x.detach().to(device=device, dtype=torch.float64)
        self.B, self.V = x.shape
        nan = torch.isnan(x)
        xs = x.masked_fill(nan, float("-inf"))  # NaN ranks with -inf: both have no mass
        self.sx, self.si = torch.sort(xs, dim=-1, descending=True, stable=True)
        self.rank_of = torch.empty_like(self.si)
        ar = torch.arange(self.V, device=x.device).expand(self.B, self.V)
        self.rank_of.scatter_(1, self.si, ar)
        top = self.sx[:, :1]
        holds = (xs == top) & (~nan | nan.all(dim=-1, keepdim=True))
        self.first = torch.where(holds, ar, self.V).min(dim=-1).values  # greedy under the total order
        self.finite = torch.isfinite(top[:, 0])
        self._ar = ar

    def intervals(self, T: float, k: int, p: float):
        """(keep [B, V] bool, lo, hi [B, V] fp64) in ranking order: the kept set and each token's CDF
        interval [lo, hi) over the renormalised kept mass. Rows with a non-finite maximum are not meant."""
        sz = self.sx / T
        keep = torch.ones_like(sz, dtype=torch.bool)
        if 0 < k < self.V:
            keep = sz >= sz[:, k - 1:k]
        w = torch.exp(sz - sz[:, :1].masked_fill(~self.finite[:, None], 0.0))
        w = torch.where(keep & torch.isfinite(w), w, torch.zeros_like(w))
        zero = torch.zeros(self.B, 1, dtype=w.dtype, device=w.device)
        if p < 1.0:
            cum = torch.cumsum(w, dim=-1)
            before = torch.cat([zero, cum[:, :-1]], dim=-1)
            drop = before >= p * cum[:, -1:]
            drop[:, 0] = False
            keep = keep & ~drop
            w = torch.where(keep, w, torch.zeros_like(w))
        cum = torch.cumsum(w, dim=-1)
        hi = cum / cum[:, -1:]
        lo = torch.cat([zero, hi[:, :-1]], dim=-1)
        return keep, lo, hi

    def token(self, u: torch.Tensor, T: float, k: int = 0, p: float = 1.0) -> torch.Tensor:
        """The rule's token per row (exact fp64)."""
        if T == 0:
            return self.first.clone()
        u = u.to(self.sx.device, torch.float64)
        keep, lo, hi = self.intervals(T, k, p)
        hit = keep & (hi > u[:, None])
        idx = torch.where(hit, self._ar, self.V).min(dim=-1).values
        last = torch.where(keep, self._ar, -1).max(dim=-1).values
        idx = torch.where(idx < self.V, idx, last)
        tok = self.si.gather(1, idx[:, None])[:, 0]
        return torch.where(self.finite, tok, self.first)

    def _nuclei(self, p: float, delta: float):
        out = [p]
        if p < 1.0:
            out += [max(p - delta, 2.0 ** -60), min(p + delta, 1.0)]
        elif delta > 0:
            out += [1.0 - delta]
        return out

    def accepted(self, tok: torch.Tensor, u: torch.Tensor, T: float, k: int = 0, p: float = 1.0,
                 delta: float = DELTA) -> torch.Tensor:
        """bool [B]: is tok[b] an acceptable draw of row b (module docstring)?"""
        tok = tok.to(self.sx.device, torch.long)
        exact = tok == self.first
        if T == 0:
            return exact
        ok = torch.zeros(self.B, dtype=torch.bool, device=self.sx.device)
        inside = (tok >= 0) & (tok < self.V)
        r = self.rank_of.gather(1, tok.clamp(0, self.V - 1)[:, None])
        u = u.to(self.sx.device, torch.float64)
        for q in self._nuclei(p, delta):
            keep, lo, hi = self.intervals(T, k, q)
            kept = keep.gather(1, r)[:, 0]
            a, b = lo.gather(1, r)[:, 0], hi.gather(1, r)[:, 0]
            ok |= kept & (a - delta <= u) & (u <= b + delta)
        return torch.where(self.finite, ok & inside, exact)

    def near_boundary(self, u: torch.Tensor, T: float, k: int = 0, p: float = 1.0,
                      delta: float = DELTA) -> torch.Tensor:
        """bool [B]: u[b] lies within delta of a CDF boundary of row b's kept set (T > 0, finite rows)."""
        u = u.to(self.sx.device, torch.float64)
        keep, lo, hi = self.intervals(T, k, p)
        edge = keep & ((hi - u[:, None]).abs() <= delta)
        return edge.any(dim=-1)


# ---- seeded defects: samplers that break the rule in one way each. The check must reject each at least once.
def defect_token(name: str, rk: Ranking, u: torch.Tensor, T: float, k: int, p: float) -> torch.Tensor:
    if name == "temperature_ignored":
        return rk.token(u, 1.0, k, p)
    if name == "top_k_ignored":
        return rk.token(u, T, 0, p)
    if name == "top_p_ignored":
        return rk.token(u, T, k, 1.0)
    if name == "u_mirrored":
        return rk.token(1.0 - u, T, k, p)
    if name == "k_off_by_one":
        return rk.token(u, T, k + 1 if k > 0 else 0, p)
    raise KeyError(name)


DEFECTS = ("temperature_ignored", "top_k_ignored", "top_p_ignored", "u_mirrored", "k_off_by_one")

# ---- inputs
KINDS = ("normal", "all_equal", "peaked", "ties")
VOCABS = (1, 7, 257, 2051, 32000, 128256)
SETTINGS = ((0.7, 0, 1.0), (1.0, 50, 1.0), (1.3, 0, 0.95), (0.7, 50, 0.5), (0.05, 5, 0.95))  # (T, top_k, top_p)


def make_logits(kind: str, B: int, V: int, dtype: torch.dtype, seed: int) -> torch.Tensor:
    """[B, V] logits of one recipe, generated on the CPU from ``seed``."""
    g = torch.Generator().manual_seed(seed)
    if kind == "normal":
        x = torch.randn(B, V, generator=g) * 3.0
    elif kind == "all_equal":
        x = torch.full((B, V), 1.5)
    elif kind == "peaked":
        x = torch.randn(B, V, generator=g)
        at = torch.randint(0, V, (B,), generator=g)
        x[torch.arange(B), at] += 12.0
    elif kind == "ties":  # four values, two of them neighbours in bf16 and fp16
        vals = torch.tensor([-1.0, 0.5, 0.50390625, 2.0])
        x = vals[torch.randint(0, 4, (B, V), generator=g)]
    else:
        raise KeyError(kind)
    return x.to(dtype)


def nonfinite_rows(dtype):
    """(logits [6, 40], the rule's token per row)."""
    nan, inf_ = float("nan"), float("inf")
    x = torch.linspace(-2, 2, 40).repeat(6, 1)
    x[0, [30, 12]] = inf_                   # +inf is the maximum: lowest id holding it
    x[1, 3] = nan                           # a NaN ranks below everything: ignored, the row samples normally
    x[1, 39] = 30.0
    x[2] = -inf_                            # all -inf: id 0
    x[3] = nan                              # all NaN: id 0
    x[4] = nan
    x[4, [25, 31]] = -inf_                  # NaN < -inf: the lowest -inf
    x[5, 0], x[5, 20] = nan, inf_           # NaN beside +inf
    return x.to(dtype), [12, 39, 0, 0, 25, 20]


# ---- the frequency check the CPU and the GPU test share
FREQ_SEED, FREQ_ROWS = 2, 4096


def frequency_case(draw):
    row = torch.tensor([2.0, 1.5, 1.0, 0.5, 0.0, -0.5, -1.0, -3.0], dtype=torch.bfloat16)
    x = row.repeat(FREQ_ROWS, 1)
    pos = torch.arange(FREQ_ROWS)
    return draw(x, pos, FREQ_SEED).cpu(), Ranking(x), uniform(pos, FREQ_SEED)


def check_frequencies(tok, rk, u):
    near = rk.near_boundary(u, 1.0)
    assert int(near.sum()) <= FREQ_ROWS // 100, int(near.sum())
    want = rk.token(u, 1.0)
    assert torch.equal(tok[~near], want[~near])
    assert rk.accepted(tok, u, 1.0).all()
    _, lo, hi = rk.intervals(1.0, 0, 1.0)
    p = (hi - lo)[0]
    n = torch.bincount(tok, minlength=8).double()
    sigma = (FREQ_ROWS * p * (1 - p)).sqrt()
    assert ((n - FREQ_ROWS * p).abs() <= 5 * sigma).all(), (n.tolist(), (FREQ_ROWS * p).tolist())
