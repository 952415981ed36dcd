"""fp64 oracle and same-dtype baseline of the regularised cross-entropy (--z-loss, --label-smoothing).

Shared by tests/test_loss_reg.py (CPU) and tests/test_loss_reg_gpu.py (the HIP kernels). Inputs and
bound functions are those of tests/kernel_oracles.py.

Per valid row (label in [0, V), not ignore_index), lse = logsumexp(x):
  nll = lse - x[label], smooth = lse - mean(x), zterm = z * lse^2
  objective = ((1 - eps) * sum nll + eps * sum smooth + sum zterm) / n
  dlogits[c] = (exp(x_c - lse) * (1 + 2 z lse) - (1 - eps) [c == label] - eps / V) * g / n, 0 on other rows
stats [8] = {objective, n, sum nll / n, sum zterm / n, sum smooth / n, mean lse, max |lse|, 0}; the kernels
and ops/reference.py form sum smooth / n only with eps > 0 (the z-only kernel does not sum the logits), so
with eps = 0 that entry is 0 here too.
"""
import torch
import torch.nn.functional as F

from pyrecover_amd.ops import reference as R
from tests.kernel_oracles import (DTYPES, IGNORE, XENT_SHAPES, approx_bound, dname, err, fp32_bound, rt,  # noqa: F401
                                  ulp_at, xent_inputs)

COEFS = [(1e-4, 0.0), (0.0, 0.1), (1e-3, 0.1)]  # (z_loss, label_smoothing)
STAT_NAMES = ("objective", "n", "nll", "zterm", "smooth", "lse_mean", "lse_absmax", "zero")


def valid_rows(labels, V, ignore_index=IGNORE):
    return labels.ne(ignore_index) & labels.ge(0) & labels.lt(V)


def reg_oracle(logits, labels, gscale, z, eps, ignore_index=IGNORE):
    """lse [T], stats [8] (fp64), dlogits (storage-dtype values, fp64) for d objective = gscale."""
    x = logits.double()
    T, V = x.shape
    lse = torch.logsumexp(x, dim=-1)
    valid = valid_rows(labels, V, ignore_index)
    vd = valid.double()
    n = vd.sum()
    safe = labels.clamp(0, V - 1)
    nll = (lse - x.gather(1, safe[:, None])[:, 0]) * vd
    smooth = (lse - x.mean(-1)) * vd
    lv = lse * vd
    ce, zt = nll.sum() / n, z * lv.pow(2).sum() / n
    sv = smooth.sum() / n if eps > 0 else 0.0 * n / n
    stats = torch.stack([(1 - eps) * ce + eps * sv + zt, n, ce, zt, sv, lv.sum() / n, lv.abs().max(),
                         torch.zeros_like(n)])
    p = torch.exp(x - lse[:, None]) * (1 + 2 * z * lse)[:, None] - eps / V
    p[torch.arange(T, device=x.device), safe] -= (1 - eps)
    d = p * vd[:, None] * (gscale / n)
    return lse, stats, rt(d, logits.dtype)


def reg_base(logits, labels, gscale, z, eps, ignore_index=IGNORE):
    """The project's same-dtype reference: cross_entropy_reg_ref + autograd in fp32 opmath.
    Returns lse, stats [8], dlogits (storage dtype)."""
    with torch.enable_grad():
        lf = R.up(logits).detach().clone().requires_grad_()
        obj, stats = R.cross_entropy_reg_ref(lf, labels, ignore_index, z, eps)
        obj.backward()
    return torch.logsumexp(R.up(logits), dim=-1), stats, (gscale * lf.grad).to(logits.dtype)


def torch_objective(x64, labels, z, eps, ignore_index=IGNORE):
    """F.cross_entropy(label_smoothing=eps) + the z term, differentiable, on fp64 logits (labels in range or
    ignore_index)."""
    valid = labels.ne(ignore_index)
    n = valid.sum()
    ce = F.cross_entropy(x64, labels, ignore_index=ignore_index, label_smoothing=eps, reduction="sum")
    lse = torch.logsumexp(x64, dim=-1)
    return (ce + z * (lse.pow(2) * valid.double()).sum()) / n
