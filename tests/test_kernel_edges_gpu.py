"""Edge shapes and dtypes of the norm, loss, elementwise and AdamW kernels against fp64 oracles.

tests/test_kernels_gpu.py runs these kernels at one or two bf16 shapes; here every dispatch arm, every
grid-stride loop's second trip, the scalar tails, strided views and bf16 / fp16 / fp32 are run at the
smallest sizes that reach them (tests/kernel_oracles.py has the oracles, baselines, recipes and bounds;
tests/test_kernel_oracles.py validates the recipes on the CPU).

  16-bit storage: max|kernel - oracle| <= 2 * max|baseline - oracle| + 1 ulp at max|oracle|
  fp32 storage:   max|kernel - oracle| <= min(4 * measured, 2^-16) * max|oracle|
  exact ops:      torch.equal

fp32-storage error of the kernels, max|kernel - oracle| / max|oracle| over all cases of this module,
measured on an MI355X (the kernels take exp, rsqrt and the reciprocal from the hardware; rstd, mean, lse
and the loss are fp32 whatever the input dtype, so their rows cover all three input dtypes):

  output              measured
  ------------------  --------
  rmsnorm.y           2.10e-07
  rmsnorm.rstd        1.38e-07
  rmsnorm.dx          1.09e-07
  rmsnorm.dw          2.23e-07
  layernorm.y         2.18e-07
  layernorm.mean      1.64e-07
  layernorm.rstd      1.36e-07
  layernorm.dx        1.73e-07
  layernorm.dw        2.04e-07
  layernorm.db        2.28e-07
  xent.lse            4.38e-08
  xent.loss           8.01e-08
  xent.dlogits        2.63e-07
  rope.x              1.09e-07
  swiglu.y            7.51e-08
  swiglu.dg           1.04e-07
  swiglu.du           6.79e-08

The inputs come from seeded CPU generators, so these figures repeat run to run.
"""
import math

import pytest
import torch

from pyrecover_amd import _ext
from pyrecover_amd.ops import reference as R
from tests import kernel_oracles as K

pytestmark = pytest.mark.gpu

F32 = torch.float32
# the table above; the bound is 4x these, never above 2^-16 (kernel_oracles.fp32_bound)
FP32_MEASURED = {
    "rmsnorm.y": 2.10e-07, "rmsnorm.rstd": 1.38e-07, "rmsnorm.dx": 1.09e-07, "rmsnorm.dw": 2.23e-07,
    "layernorm.y": 2.18e-07, "layernorm.mean": 1.64e-07, "layernorm.rstd": 1.36e-07, "layernorm.dx": 1.73e-07,
    "layernorm.dw": 2.04e-07, "layernorm.db": 2.28e-07,
    "xent.lse": 4.38e-08, "xent.loss": 8.01e-08, "xent.dlogits": 2.63e-07,
    "rope.x": 1.09e-07,
    "swiglu.y": 7.51e-08, "swiglu.dg": 1.04e-07, "swiglu.du": 6.79e-08,
}


def _check(key, got, base, oracle, storage):
    """Print the figures, then assert the bound of the storage dtype."""
    e = K.err(got, oracle)
    mx = oracle.abs().max().item()
    bound = K.fp32_bound(FP32_MEASURED[key], oracle) if storage == F32 else K.approx_bound(storage, base, oracle)
    print(f"ERR {key} {K.dname(storage)} err={e:.3e} rel={e / max(mx, 1e-300):.3e} base={K.err(base, oracle):.3e} "
          f"bound={bound:.3e}")
    assert torch.isfinite(got.double()).all(), key
    assert e <= bound, (key, e, bound)


# ------------------------------------------------------------------------------------------------
# RMSNorm / LayerNorm: forward NV = 1, 2, 4, 8, 16 and backward NVB = 1, 2, 4 (D <= 8192 is the forward's
# limit), D that is no multiple of a 512 / 2048-element chunk, rows % 4 != 0, more rows than backward blocks
# (1025, 2051: a block walks 2-3 rows), fewer partial rows than the column sum's 16 slices (1, 3, 15).
@pytest.mark.parametrize("rows,D", K.NORM_SHAPES)
@pytest.mark.parametrize("dtype", K.DTYPES, ids=K.dname)
def test_rmsnorm_edges(cuda, rows, D, dtype):
    C = _ext.native()
    x, delta, w, _, dy, dres, dwb0 = K.norm_inputs(rows, D, dtype, cuda)
    for with_delta in (False, True):
        d, dr = (delta, dres) if with_delta else (None, None)
        h, y, rstd = C.rmsnorm_fwd(x, d, w, K.EPS)
        hb, yb, rb = K.rmsnorm_fwd_base(x, d, w)
        ho, yo, ro = K.rmsnorm_fwd_oracle(x, d, w)
        assert torch.equal(h, hb) and torch.equal(h.double(), ho)
        _check("rmsnorm.y", y, yb, yo, dtype)
        _check("rmsnorm.rstd", rstd, rb, ro, F32)
        if dtype == torch.bfloat16 and rows * D >= 1000:  # a share needs a sample: one element of 8 is 12%
            assert (y != yb).float().mean().item() < 0.01
        for dw0 in (None, dwb0[:D]):
            outs = []
            for _ in range(2):
                dw = torch.full_like(w, float("nan")) if dw0 is None else dw0.clone()
                outs.append((C.rmsnorm_bwd(dy, h, w, rstd, dr, dw, dw0 is not None), dw))
            (dx, dw), (dx2, dw2) = outs
            assert torch.equal(dw, dw2) and torch.equal(dx, dx2)  # bit-equal run to run
            dxb, dwb = K.rmsnorm_bwd_base(dy, h, w, rstd, dr, dw0)
            dxo, dwo = K.rmsnorm_bwd_oracle(dy, h, w, rstd, dr, dw0)
            _check("rmsnorm.dx", dx, dxb, dxo, dtype)
            _check("rmsnorm.dw", dw, dwb, dwo, dtype)


@pytest.mark.parametrize("rows,D", K.NORM_SHAPES)
@pytest.mark.parametrize("dtype", K.DTYPES, ids=K.dname)
def test_layernorm_edges(cuda, rows, D, dtype):
    C = _ext.native()
    x, delta, w, b, dy, dres, dwb0 = K.norm_inputs(rows, D, dtype, cuda, layernorm=True)
    for with_delta in (False, True):
        d, dr = (delta, dres) if with_delta else (None, None)
        h, y, mean, rstd = C.layernorm_fwd(x, d, w, b, K.EPS)
        hb, yb, mb, rb = K.layernorm_fwd_base(x, d, w, b)
        ho, yo, mo, ro = K.layernorm_fwd_oracle(x, d, w, b)
        assert torch.equal(h, hb) and torch.equal(h.double(), ho)
        _check("layernorm.y", y, yb, yo, dtype)
        _check("layernorm.mean", mean, mb, mo, F32)
        _check("layernorm.rstd", rstd, rb, ro, F32)
        for acc0 in (None, dwb0):
            outs = []
            for _ in range(2):
                dwb = torch.full_like(dwb0, float("nan")) if acc0 is None else acc0.clone()
                outs.append((C.layernorm_bwd(dy, h, w, mean, rstd, dr, dwb, acc0 is not None), dwb))
            (dx, dwb), (dx2, dwb2) = outs
            assert torch.equal(dwb, dwb2) and torch.equal(dx, dx2)
            dxb, dwbb = K.layernorm_bwd_base(dy, h, w, b, dr, acc0)
            dxo, dwbo = K.layernorm_bwd_oracle(dy, h, w, mean, rstd, dr, acc0)
            _check("layernorm.dx", dx, dxb, dxo, dtype)
            _check("layernorm.dw", dwb[:D], dwbb[:D], dwbo[:D], dtype)
            _check("layernorm.db", dwb[D:], dwbb[D:], dwbo[D:], dtype)


@pytest.mark.parametrize("D", [8200, 12])
def test_norms_reject_unsupported_width(cuda, D):
    """D > 8192 (the forward holds a row in registers) and D % 8 != 0 (16-B vectors) raise from the binding."""
    C = _ext.native()
    x = torch.randn(4, D, device=cuda, dtype=torch.bfloat16)
    w, b = torch.ones(D, device=cuda, dtype=torch.bfloat16), torch.zeros(D, device=cuda, dtype=torch.bfloat16)
    st = torch.ones(4, device=cuda)
    rule = "multiple of 8 and <= 8192"
    with pytest.raises(RuntimeError, match=rule):
        C.rmsnorm_fwd(x, None, w, K.EPS)
    with pytest.raises(RuntimeError, match=rule):
        C.layernorm_fwd(x, None, w, b, K.EPS)
    with pytest.raises(RuntimeError, match=rule):
        C.rmsnorm_bwd(x, x, w, st, None, torch.empty_like(w), False)
    with pytest.raises(RuntimeError, match=rule):
        C.layernorm_bwd(x, x, w, st, st, None, torch.empty(2 * D, device=cuda, dtype=torch.bfloat16), False)


# ------------------------------------------------------------------------------------------------
# Cross-entropy: V % 8 != 0 (scalar tail), row stride != V, V < 2048 (lanes that hold m = -inf)
def _xent_run(C, buf, V, labels, g):
    work = buf.clone()
    lg = work[:, :V]
    lse, _, stats = C.xent_fwd(lg, labels, K.IGNORE)
    stats0 = stats.clone()
    C.xent_bwd_(lg, labels, lse, stats, g, K.IGNORE)
    assert torch.equal(work[:, V:], buf[:, V:])  # padding columns bit-unchanged
    return lse, stats0, lg


@pytest.mark.parametrize("T,V,ld", K.XENT_SHAPES)
@pytest.mark.parametrize("dtype", K.DTYPES, ids=K.dname)
def test_cross_entropy_edges(cuda, T, V, ld, dtype):
    C = _ext.native()
    buf, logits, labels = K.xent_inputs(T, V, ld, dtype, cuda)
    g = torch.full((1,), 0.5, device=cuda)
    for row0_ignored in (False, True):
        lab = labels.clone()
        if row0_ignored:
            lab[0] = K.IGNORE
        lse, stats, d = _xent_run(C, buf, V, lab, g)
        lb, lossb, db = K.xent_base(logits, lab, 0.5)
        lo, losso, n, do = K.xent_oracle(logits, lab, 0.5)
        _check("xent.lse", lse, lb, lo, F32)
        _check("xent.loss", stats[0], lossb, losso, F32)
        assert stats[1].item() == n
        _check("xent.dlogits", d, db, do, dtype)
        if (lab == K.IGNORE).any():
            assert d[lab == K.IGNORE].abs().max().item() == 0


@pytest.mark.parametrize("T,V,ld", [(7, 1001, 1008), (4, 2049, 2056)])
@pytest.mark.parametrize("dtype", K.DTYPES, ids=K.dname)
def test_cross_entropy_out_of_range_labels_are_ignored(cuda, T, V, ld, dtype):
    """A label outside [0, V) other than ignore_index: loss 0, not counted, zero gradient row -- the
    results of the same batch with those labels set to ignore_index, bit for bit, and its oracle."""
    C = _ext.native()
    buf, logits, labels = K.xent_inputs(T, V, ld, dtype, cuda)
    g = torch.full((1,), 0.5, device=cuda)
    bad, same = labels.clone(), labels.clone()
    bad[0], bad[1] = V, -7
    same[0] = same[1] = K.IGNORE
    lse, stats, d = _xent_run(C, buf, V, bad, g)
    lse2, stats2, d2 = _xent_run(C, buf, V, same, g)
    assert torch.equal(lse, lse2) and torch.equal(stats, stats2) and torch.equal(d, d2)
    lb, lossb, db = K.xent_base(logits, same, 0.5)
    lo, losso, n, do = K.xent_oracle(logits, same, 0.5)
    assert stats[1].item() == n == T - 3
    _check("xent.loss", stats[0], lossb, losso, F32)
    _check("xent.dlogits", d, db, do, dtype)
    assert d[:3].abs().max().item() == 0


@pytest.mark.parametrize("dtype", K.DTYPES, ids=K.dname)
def test_cross_entropy_all_ignored(cuda, dtype):
    """No valid label: NaN loss, as cross_entropy_ref gives, and all-zero dlogits."""
    C = _ext.native()
    T, V, ld = 4, 2049, 2056
    buf, logits, labels = K.xent_inputs(T, V, ld, dtype, cuda)
    labels.fill_(K.IGNORE)
    assert math.isnan(R.cross_entropy_ref(logits, labels).item())
    lse, stats, d = _xent_run(C, buf, V, labels, torch.full((1,), 0.5, device=cuda))
    assert math.isnan(stats[0].item()) and stats[1].item() == 0
    assert d.abs().max().item() == 0
    _check("xent.lse", lse, torch.logsumexp(R.up(logits), -1), torch.logsumexp(logits.double(), -1), F32)


def test_cross_entropy_rejects_unpadded_rows(cuda):
    """A contiguous [T, 1001] tensor has rows that are not 16-B vectors apart: the error names the rule."""
    C = _ext.native()
    logits = torch.randn(4, 1001, device=cuda, dtype=torch.bfloat16)
    labels = torch.zeros(4, dtype=torch.long, device=cuda)
    with pytest.raises(RuntimeError, match=r"row stride % 8"):
        C.xent_fwd(logits, labels, K.IGNORE)
    f = torch.zeros(4, device=cuda)
    with pytest.raises(RuntimeError, match=r"row stride % 8"):
        C.xent_bwd_(logits, labels, f, f[:2], f[:1], K.IGNORE)


# ------------------------------------------------------------------------------------------------
# RoPE: 4096 x 160 = 655,360 work items > 2048 blocks x 256 (the grid-stride loop repeats), the rotated
# columns inside a wider row, pos_offset, head_dim 128 / 64 / 8
@pytest.mark.parametrize("ntok,S,ncols,D", K.ROPE_SHAPES)
@pytest.mark.parametrize("dtype", K.DTYPES, ids=K.dname)
def test_rope_edges(cuda, ntok, S, ncols, D, dtype):
    C = _ext.native()
    buf, tab = K.rope_inputs(ntok, S, ncols, D, dtype, cuda)
    for pos_offset in (0, K.ROPE_MAX_OFFSET):
        for inverse in (False, True):
            work = buf.clone()
            x = work[:, 8:]
            C.rope_(x, ncols, tab, D, S, pos_offset, inverse)
            src = buf[:, 8:]
            _check("rope.x", x[:, :ncols], K.rope_base(src, ncols, tab, D, S, pos_offset, inverse),
                   K.rope_oracle(src, ncols, tab, D, S, pos_offset, inverse), dtype)
            assert torch.equal(work[:, :8], buf[:, :8]) and torch.equal(x[:, ncols:], src[:, ncols:])


# ------------------------------------------------------------------------------------------------
# SwiGLU forward and backward variant 0: 2050 x 257 = 526,850 work items > 524,288, gu a column view
@pytest.mark.parametrize("dtype", K.DTYPES, ids=K.dname)
def test_swiglu_edges(cuda, dtype):
    C = _ext.native()
    T, Fd = K.SWIGLU_SHAPE
    gbuf, dbuf, obuf = K.swiglu_inputs(T, Fd, dtype, cuda)
    gu, dy = gbuf[:, 8:8 + 2 * Fd], dbuf[:, 8:8 + Fd]
    g, u = gu[:, :Fd], gu[:, Fd:]
    gkeep = gbuf.clone()
    y = C.swiglu_fwd(gu)
    _check("swiglu.y", y, R.swiglu_ref(g, u), K.swiglu_fwd_oracle(g, u), dtype)
    out = obuf.clone()
    ov = out[:, 8:8 + 2 * Fd]
    C.swiglu_bwd(dy, gu, ov, 0)
    dgb, dub = R.swiglu_bwd_ref(dy, g, u)
    dgo, duo = K.swiglu_bwd_oracle(dy, g, u)
    _check("swiglu.dg", ov[:, :Fd], dgb, dgo, dtype)
    _check("swiglu.du", ov[:, Fd:], dub, duo, dtype)
    assert torch.equal(out[:, :8], obuf[:, :8]) and torch.equal(out[:, 8 + 2 * Fd:], obuf[:, 8 + 2 * Fd:])
    assert torch.equal(gbuf, gkeep)
    inplace = gbuf.clone()  # dgu aliases gu, as the MLP backward calls it
    iv = inplace[:, 8:8 + 2 * Fd]
    C.swiglu_bwd(dy, iv, iv, 0)
    assert torch.equal(iv, ov)
    assert torch.equal(inplace[:, :8], gbuf[:, :8]) and torch.equal(inplace[:, 8 + 2 * Fd:], gbuf[:, 8 + 2 * Fd:])


# ------------------------------------------------------------------------------------------------
# Embedding: D = 8 (one lane), 520 (a partial second trip of the 512-column loop), 4096 (eight trips)
@pytest.mark.parametrize("V,D,ntok", K.EMBED_SHAPES)
@pytest.mark.parametrize("dtype", K.DTYPES, ids=K.dname)
def test_embedding_edges(cuda, V, D, ntok, dtype):
    C = _ext.native()
    W, ids, dout, dW0 = K.embed_inputs(V, D, ntok, dtype, cuda)
    assert torch.equal(C.embedding_fwd(ids, W), W[ids])
    untouched = torch.ones(V, dtype=torch.bool, device=cuda)
    untouched[ids] = False
    assert untouched.any()
    for acc0 in (None, dW0):
        outs = []
        for _ in range(2):
            dW = torch.full_like(W, float("nan")) if acc0 is None else acc0.clone()
            C.embedding_bwd(ids, dout, dW, acc0 is not None)
            outs.append(dW)
        assert torch.equal(outs[0], outs[1])
        # fp32 sums of these inputs are exact: the rounded fp64 index_add_, bit for bit
        assert torch.equal(outs[0].double(), K.embed_bwd_oracle(ids, dout, V, acc0))
        if acc0 is not None:
            assert torch.equal(outs[0][untouched], dW0[untouched])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=K.dname)
def test_embedding_out_of_range_ids(cuda, dtype):
    """Ids -1 and V read row 0 in the forward and are dropped in the backward (elementwise.hip says so)."""
    C = _ext.native()
    V, D, ntok = 50, 520, 4099
    W, ids, dout, dW0 = K.embed_inputs(V, D, ntok, dtype, cuda)
    ids[0], ids[7], ids[-1] = -1, V, V
    out = C.embedding_fwd(ids, W)
    bad = (ids < 0) | (ids >= V)
    assert torch.equal(out[~bad], W[ids[~bad]]) and torch.equal(out[bad], W[:1].expand(3, D))
    for acc0 in (None, dW0):
        dW = torch.full_like(W, float("nan")) if acc0 is None else acc0.clone()
        C.embedding_bwd(ids, dout, dW, acc0 is not None)
        assert torch.equal(dW.double(), K.embed_bwd_oracle(ids, dout, V, acc0))


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", K.GRAD_NORM_SIZES)
@pytest.mark.parametrize("dtype", K.DTYPES, ids=K.dname)
def test_grad_norm_edges(cuda, n, dtype):
    C = _ext.native()
    x = K.grad_norm_input(n, dtype, cuda)
    o = K.grad_norm_oracle(x)
    for max_norm in (0.25 * o, 4.0 * o, 0.0, -1.0):
        out = C.grad_norm(x, max_norm, K.GRAD_NORM_PRE_SCALE)
        print(f"ERR grad_norm n={n} max_norm={max_norm:.3e} norm={out[0].item():.9e} oracle={o:.9e} coef={out[1].item()}")
        assert abs(out[0].item() - o) <= 1e-3 * o
        if 0 < max_norm < o:  # norm above max_norm: coefficient max_norm / (norm + 1e-6)
            want = max_norm / (o + 1e-6)
            assert abs(out[1].item() - want) <= 1e-3 * want and out[1].item() < 1.0
        else:  # norm below max_norm, or clipping off: exactly 1
            assert out[1].item() == 1.0


# ------------------------------------------------------------------------------------------------
# AdamW. adamw16_kernel repeats its loop for n / 8 > 4096 * 512, adamw_kernel (fp32) and
# adamw_master_kernel for n / 8 > 4096 * 256; both big sizes end in a partial second trip, a second chunk
# that is partly past the end, and a scalar tail of 5.
ADAM_SMALL = [1, 7, 8, 9, 4099]
ADAM_BIG16 = (1 << 24) + 4096 + 5
ADAM_BIG32 = (1 << 23) + 2048 + 5
LR, B1, B2, AEPS, WD = 1e-3, 0.9, 0.999, 1e-8, 0.01
KINDS = [("flat", torch.bfloat16), ("flat", torch.float16), ("flat", torch.float32), ("master", torch.bfloat16),
         ("master", torch.float16)]
KIND_IDS = [f"{k}-{K.dname(d)}" for k, d in KINDS]


def _adam_sizes(kind, dtype):
    return ADAM_SMALL + [ADAM_BIG16 if (kind == "flat" and dtype != F32) else ADAM_BIG32]


def _adam_state(kind, n, dtype, cuda):
    """p (16-bit or fp32), pm (fp32 master or None), non-zero m and v, three gradients."""
    g = torch.Generator(device=cuda).manual_seed(n)
    sdt = F32 if kind == "master" else dtype
    pm = torch.randn(n, device=cuda, generator=g)
    m = (torch.randn(n, device=cuda, generator=g) * 1e-3).to(sdt)
    v = (torch.rand(n, device=cuda, generator=g) * 1e-4).to(sdt)
    grads = [(torch.randn(n, device=cuda, generator=g) * 10.0 ** (-s)).to(dtype) for s in (1, 2, 3)]
    return pm.to(dtype), (pm if kind == "master" else None), m, v, grads


def _adam_step(C, kind, st, grad, s, gscale=1.0, gscale_dev=None, hyper_dev=None, fast=False):
    p, pm, m, v = st
    bc1, bc2s = 1 - B1 ** s, math.sqrt(1 - B2 ** s)
    if kind == "master":
        C.adamw_master_(p, pm, grad, m, v, LR, B1, B2, AEPS, WD, bc1, bc2s, gscale, gscale_dev, hyper_dev, fast)
    else:
        C.adamw_flat_(p, grad, m, v, LR, B1, B2, AEPS, WD, bc1, bc2s, gscale, gscale_dev, hyper_dev, fast)


def _adam_ours(C, kind, state, fast, cuda, device_scalars=False, gscale=1.0):
    p, pm, m, v, grads = state
    st = (p.clone(), None if pm is None else pm.clone(), m.clone(), v.clone())
    for s, grad in enumerate(grads, 1):
        if device_scalars:  # gscale and {lr, bc1, bc2_sqrt} from device memory, host arguments neutral / unused
            gs = torch.tensor([gscale], device=cuda)
            hy = torch.tensor([LR, 1 - B1 ** s, math.sqrt(1 - B2 ** s)], device=cuda, dtype=torch.float64)
            p_, pm_, m_, v_ = st
            if kind == "master":
                C.adamw_master_(p_, pm_, grad, m_, v_, 7.0, B1, B2, AEPS, WD, 0.3, 0.3, 1.0, gs, hy, fast)
            else:
                C.adamw_flat_(p_, grad, m_, v_, 7.0, B1, B2, AEPS, WD, 0.3, 0.3, 1.0, gs, hy, fast)
        else:
            _adam_step(C, kind, st, grad, s, gscale=gscale, fast=fast)
    return st


def _adam_torch(kind, state, cuda):
    """torch's fused AdamW on the same state (fp32 state and widened gradients for the master kernel)."""
    p, pm, m, v, grads = state
    p2 = (pm if kind == "master" else p).clone()
    m2, v2 = m.clone(), v.clone()
    step = torch.zeros((), device=cuda)
    for grad in grads:
        step += 1
        torch._fused_adamw_([p2], [grad.to(p2.dtype)], [m2], [v2], [], [step], amsgrad=False, lr=LR, beta1=B1,
                            beta2=B2, weight_decay=WD, eps=AEPS, maximize=False)
    return p2, m2, v2


def _first_diff(a, b):
    bad = (a != b).nonzero()
    return bad.numel(), bad[:4].flatten().tolist()


def _adam_sizes_params():
    return [pytest.param(k, d, n, id=f"{k}-{K.dname(d)}-{n}") for k, d in KINDS for n in _adam_sizes(k, d)]


@pytest.mark.parametrize("kind,dtype,n", _adam_sizes_params())
def test_adamw_exact(cuda, kind, dtype, n):
    """Three steps from non-zero moments: the default math is bit-equal to torch._fused_adamw_ on p, m and
    v (for the master kernel: on the fp32 master, and p is the master rounded once); with either math the
    device-scalar path is bit-equal to the host-scalar path."""
    C = _ext.native()
    state = _adam_state(kind, n, dtype, cuda)
    p, pm, m, v = _adam_ours(C, kind, state, False, cuda)
    p2, m2, v2 = _adam_torch(kind, state, cuda)
    for name, a, b in (("p", pm if kind == "master" else p, p2), ("m", m, m2), ("v", v, v2)):
        assert torch.equal(a, b), (name, _first_diff(a, b))
    if kind == "master":
        assert torch.equal(p, pm.to(dtype))
    for fast in (False, True):
        host = _adam_ours(C, kind, state, fast, cuda, gscale=0.5)
        dev = _adam_ours(C, kind, state, fast, cuda, device_scalars=True, gscale=0.5)
        for a, b in zip(host, dev):
            assert a is None or torch.equal(a, b), (fast, _first_diff(a, b))
        if n >= 4099 and not fast:
            assert not torch.equal(host[0], p)  # the gradient scale took effect


@pytest.mark.parametrize("kind,dtype", KINDS, ids=KIND_IDS)
def test_adamw_fast_tracks_torch(cuda, kind, dtype):
    """fast=True (hardware reciprocal / square root): p, m, v within 1e-2 of torch's at every size, and for
    16-bit parameters under 1e-3 of them differ at all -- a share, so it is taken over all sizes together
    (one element of n = 7 is already 14%)."""
    C = _ext.native()
    differ = total = 0
    for n in _adam_sizes(kind, dtype):
        state = _adam_state(kind, n, dtype, cuda)
        p, pm, m, v = _adam_ours(C, kind, state, True, cuda)
        p2, m2, v2 = _adam_torch(kind, state, cuda)
        for name, a, b in (("p", pm if kind == "master" else p, p2), ("m", m, m2), ("v", v, v2)):
            rel = ((a.float() - b.float()).abs().max() / b.float().abs().max().clamp_min(1e-6)).item()
            print(f"ERR adamw_fast {kind} {K.dname(dtype)} n={n} {name} rel={rel:.3e}")
            assert rel < 1e-2, (n, name, rel)
        ref16 = p2.to(dtype)
        differ += (p != ref16).sum().item()
        total += n
    print(f"ERR adamw_fast {kind} {K.dname(dtype)} share={differ / total:.3e}")
    if dtype != F32:
        assert differ / total < 1e-3


@pytest.mark.parametrize("kind,dtype", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("fast", [False, True])
def test_adamw_on_slices_leaves_guards(cuda, kind, dtype, fast):
    """The update of big[off : off + n] (off a multiple of 64: the ZeRO-1 chunk grid of parallel/flat.py)
    equals the update of a stand-alone copy and leaves every buffer bit-unchanged before and after."""
    C = _ext.native()
    n, off, pad = 4099, 192, 333
    state = _adam_state(kind, off + n + pad, dtype, cuda)
    p, pm, m, v, grads = state
    grad = grads[0]
    bufs = [t for t in (p, pm, grad, m, v) if t is not None]
    keep = [t.clone() for t in bufs]
    alone = [t[off:off + n].clone() for t in bufs]
    sl = [t[off:off + n] for t in bufs]

    def run(ts):
        if kind == "master":
            pp, pmm, gg, mm, vv = ts
        else:
            (pp, gg, mm, vv), pmm = ts, None
        _adam_step(C, kind, (pp, pmm, mm, vv), gg, 2, gscale=0.5, fast=fast)

    run(sl)
    run(alone)
    for big, k, a in zip(bufs, keep, alone):
        assert torch.equal(big[off:off + n], a)
        assert torch.equal(big[:off], k[:off]) and torch.equal(big[off + n:], k[off + n:])
    assert not torch.equal(p[off:off + n], keep[0][off:off + n])


def test_adamw_bindings_reject_bad_device_scalars(cuda):
    """Each of the five AdamW entry points refuses every optional device scalar it takes (gscale_dev fp32[1],
    hyper_dev fp64[3], skip_dev int32[1], and step_dev int32[1] for the stochastic-rounding ones) when it has
    the wrong dtype, too few elements or lives on the host, before anything is launched: the state stays
    bit-equal. The host tensor comes last in each group, after the harmless cases. A valid call with all of
    them then updates p."""
    C = _ext.native()
    bf, i32 = torch.bfloat16, torch.int32
    gen = torch.Generator(device=cuda).manual_seed(11)
    # lr = 1: one step moves p by about 0.03, several bf16 ulps, also where p is the fp32 master rounded
    co = (1.0, B1, B2, AEPS, WD, 1 - B1, math.sqrt(1 - B2), 1.0)
    sr = dict(seed=1, base=0, step=1, mask=7)

    def rnd(shape, dtype, scale=1.0):
        return (torch.randn(shape, device=cuda, generator=gen) * scale).to(dtype)

    def state(shape, sdt):  # p, g, m, v
        return [rnd(shape, bf), rnd(shape, bf, 0.1), rnd(shape, sdt, 1e-3), rnd(shape, sdt, 1e-2).abs()]

    flat, mat = state(64, bf), state((64, 64), bf)
    p, g, m, v = state(64, F32)
    master = [p, p.float(), g, m, v]  # p, pm, g, m, v
    entries = [("flat", C.adamw_flat_, flat, {}), ("master", C.adamw_master_, master, {}),
               ("t", C.adamw_t_, mat + [torch.zeros(64, 64, dtype=bf, device=cuda)], {}),
               ("flat_sr", C.adamw_flat_sr_, [t.clone() for t in flat], sr),
               ("t_sr", C.adamw_t_sr_, [t.clone() for t in mat] + [torch.zeros(64, 64, dtype=bf, device=cuda)], sr)]
    # name: (valid values, dtype, a wrong dtype, too few elements)
    scalars = {"gscale_dev": ([1.0], F32, torch.float64, 0), "hyper_dev": ([co[0], co[5], co[6]], torch.float64, F32, 2),
               "skip_dev": ([0], i32, torch.int64, 0), "step_dev": ([1], i32, torch.int64, 0)}
    for kind, fn, tensors, extra in entries:
        keep = [t.clone() for t in tensors]
        names = [k for k in scalars if k != "step_dev" or extra]
        for name in names:
            vals, dtype, wrong, few = scalars[name]
            bad = [("dtype", torch.tensor(vals, dtype=wrong, device=cuda)),
                   ("size", torch.tensor(vals[:few], dtype=dtype, device=cuda)),
                   ("host", torch.tensor(vals, dtype=dtype))]
            for what, t in bad:
                with pytest.raises(RuntimeError):
                    fn(*tensors, *co, **{**extra, name: t})
                    pytest.fail(f"{kind}: {name} with a bad {what} was accepted")
                for a, b in zip(tensors, keep):
                    assert torch.equal(a, b), (kind, name, what)
        good = {k: torch.tensor(scalars[k][0], dtype=scalars[k][1], device=cuda) for k in names}
        fn(*tensors, *co, **{**extra, **good})
        assert not torch.equal(tensors[0], keep[0]), kind
