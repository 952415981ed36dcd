"""The input recipes and bounds of tests/test_kernel_edges_gpu.py, validated on the CPU: for every recipe
at its small sizes, the same-dtype baseline alone must satisfy each cap the GPU test applies to the HIP
kernels (the fp32 2^-16 cap, the bf16 RMSNorm mismatch share, grad_norm's 1e-3, exact `h`), must sit
within a few ulps of the fp64 oracle (a lax baseline would make the 2x-baseline bound meaningless), and
the exact-sum embedding inputs must really sum exactly in fp32."""
import pytest
import torch

from tests import kernel_oracles as K

CPU = torch.device("cpu")
SMALL_NORM = [s for s in K.NORM_SHAPES if s[0] * s[1] <= 70000]
# A same-dtype fp32-opmath baseline differs from the rounded fp64 oracle only where an intermediate rounding
# lands on the other side of a tie: one ulp of the element, which is at most one ulp at max|oracle|; a
# second rounding (dres, accumulate) can add one more.
BASE_ULPS = 2


def _check(name, base, oracle, storage):
    e = K.err(base, oracle)
    mx = oracle.abs().max().item()
    if storage == torch.float32:
        assert e <= K.FP32_CAP * mx, (name, e, mx)
    else:
        assert e <= BASE_ULPS * K.ulp_at(storage, mx), (name, e, mx)
    assert K.approx_bound(storage, base, oracle) >= e


@pytest.mark.parametrize("rows,D", SMALL_NORM)
@pytest.mark.parametrize("dtype", K.DTYPES, ids=K.dname)
@pytest.mark.parametrize("with_delta", [False, True])
def test_rmsnorm_baseline_within_caps(rows, D, dtype, with_delta):
    x, delta, w, _, dy, dres, dwb0 = K.norm_inputs(rows, D, dtype, CPU)
    delta, dres = (delta, dres) if with_delta else (None, None)
    h, y, rstd = K.rmsnorm_fwd_base(x, delta, w)
    ho, yo, ro = K.rmsnorm_fwd_oracle(x, delta, w)
    assert torch.equal(h.double(), ho)
    _check("y", y, yo, dtype)
    _check("rstd", rstd, ro, torch.float32)
    if dtype == torch.bfloat16 and rows * D >= 1000:
        assert (y.double() != yo).double().mean().item() < 0.01
    for dw0 in (None, dwb0[:D]):
        dx, dw = K.rmsnorm_bwd_base(dy, h, w, rstd, dres, dw0)
        dxo, dwo = K.rmsnorm_bwd_oracle(dy, h, w, rstd, dres, dw0)
        _check("dx", dx, dxo, dtype)
        _check("dw", dw, dwo, dtype)


@pytest.mark.parametrize("rows,D", SMALL_NORM)
@pytest.mark.parametrize("dtype", K.DTYPES, ids=K.dname)
@pytest.mark.parametrize("with_delta", [False, True])
def test_layernorm_baseline_within_caps(rows, D, dtype, with_delta):
    x, delta, w, b, dy, dres, dwb0 = K.norm_inputs(rows, D, dtype, CPU, layernorm=True)
    delta, dres = (delta, dres) if with_delta else (None, None)
    h, y, mean, rstd = K.layernorm_fwd_base(x, delta, w, b)
    ho, yo, mo, ro = K.layernorm_fwd_oracle(x, delta, w, b)
    assert torch.equal(h.double(), ho)
    _check("y", y, yo, dtype)
    _check("mean", mean, mo, torch.float32)
    _check("rstd", rstd, ro, torch.float32)
    for dwb0_ in (None, dwb0):
        dx, dwb = K.layernorm_bwd_base(dy, h, w, b, dres, dwb0_)
        dxo, dwbo = K.layernorm_bwd_oracle(dy, h, w, mean, rstd, dres, dwb0_)
        _check("dx", dx, dxo, dtype)
        _check("dw", dwb[:D], dwbo[:D], dtype)
        _check("db", dwb[D:], dwbo[D:], dtype)


@pytest.mark.parametrize("T,V,ld", K.XENT_SHAPES)
@pytest.mark.parametrize("dtype", K.DTYPES, ids=K.dname)
def test_cross_entropy_baseline_within_caps(T, V, ld, dtype):
    buf, logits, labels = K.xent_inputs(T, V, ld, dtype, CPU)
    assert logits.stride(0) == ld and ld % 8 == 0
    assert {0, V - 1} <= set(labels.tolist()) and (T <= 2 or K.IGNORE in labels.tolist())
    assert (buf[:, V:] == torch.finfo(dtype).max).all()
    assert logits[0].float().max() >= 79 and logits[0].float().min() <= -79  # the +-80 row survived the dtype
    lse, loss, d = K.xent_base(logits, labels, 0.5)
    lo, losso, n, do = K.xent_oracle(logits, labels, 0.5)
    assert n == labels.ne(K.IGNORE).sum().item()
    _check("lse", lse, lo, torch.float32)
    _check("loss", loss, losso, torch.float32)
    _check("dlogits", d, do, dtype)
    # out-of-range labels are treated like ignore_index: the oracle the GPU test uses for them
    bad = labels.clone()
    bad[0] = V
    bad[1] = -7
    same = labels.clone()
    same[0] = same[1] = K.IGNORE
    assert K.xent_oracle(logits, same, 0.5)[2] == n - 2
    assert bad.ne(K.IGNORE).sum().item() == n  # ... which a plain `!= ignore_index` count would miss


@pytest.mark.parametrize("ntok,S,ncols,D", K.ROPE_SHAPES[1:])
@pytest.mark.parametrize("dtype", K.DTYPES, ids=K.dname)
@pytest.mark.parametrize("pos_offset", [0, K.ROPE_MAX_OFFSET])
@pytest.mark.parametrize("inverse", [False, True])
def test_rope_baseline_within_caps(ntok, S, ncols, D, dtype, pos_offset, inverse):
    buf, tab = K.rope_inputs(ntok, S, ncols, D, dtype, CPU)
    assert tab.shape[0] >= S + pos_offset
    x = buf[:, 8:]
    base = K.rope_base(x, ncols, tab, D, S, pos_offset, inverse)
    _check("x", base, K.rope_oracle(x, ncols, tab, D, S, pos_offset, inverse), dtype)


@pytest.mark.parametrize("dtype", K.DTYPES, ids=K.dname)
def test_swiglu_baseline_within_caps(dtype):
    from pyrecover_amd.ops import reference as R

    T, Fd = 67, 136  # the recipe of SWIGLU_SHAPE at a small size
    gbuf, dbuf, _ = K.swiglu_inputs(T, Fd, dtype, CPU)
    g, u, dy = gbuf[:, 8:8 + Fd], gbuf[:, 8 + Fd:8 + 2 * Fd], dbuf[:, 8:8 + Fd]
    _check("y", R.swiglu_ref(g, u), K.swiglu_fwd_oracle(g, u), dtype)
    dg, du = R.swiglu_bwd_ref(dy, g, u)
    dgo, duo = K.swiglu_bwd_oracle(dy, g, u)
    _check("dg", dg, dgo, dtype)
    _check("du", du, duo, dtype)


@pytest.mark.parametrize("V,D,ntok", [s for s in K.EMBED_SHAPES if s[1] * s[2] <= 3_000_000])
@pytest.mark.parametrize("dtype", K.DTYPES, ids=K.dname)
def test_embedding_inputs_sum_exactly_in_fp32(V, D, ntok, dtype):
    W, ids, dout, dW0 = K.embed_inputs(V, D, ntok, dtype, CPU)
    for t in (dout, dW0):  # multiples of 1/8 that the storage dtype holds exactly
        assert torch.equal((t.double() * 8).round() / 8, t.double())
    assert dout.abs().max() <= 1 and dW0.abs().max() <= 4 and dW0.abs().max() > 0
    assert (ntok + 4) * 8 < 2 ** 24  # every partial sum is an integer number of eighths below 2^24
    for acc0 in (None, dW0):
        o = K.embed_bwd_oracle(ids, dout, V, acc0)
        for order in (torch.arange(ntok), torch.arange(ntok - 1, -1, -1)):  # fp32 sums: any order, same bits
            s32 = torch.zeros(V, D) if acc0 is None else acc0.float().clone()
            s32.index_add_(0, ids[order], dout.float()[order])
            assert torch.equal(s32.to(dtype).double(), o)
    if V == 16:
        assert ids.unique().numel() == 1
    count = ids.bincount(minlength=V)
    assert (count == 0).any()  # rows no id touches, for the accumulate guard
    if (V, ntok) == (50, 4099):
        assert count[count > 0].min() > 40 and count[0] > 0 and count[V - 1] > 0  # heavy in duplicates
    # ids -1 and V are dropped by the oracle
    ids2 = ids.clone()
    ids2[0], ids2[-1] = -1, V
    o2 = K.embed_bwd_oracle(ids2, dout, V, None)
    assert torch.equal(o2, K.embed_bwd_oracle(ids[1:-1], dout[1:-1], V, None))


@pytest.mark.parametrize("n", K.GRAD_NORM_SIZES)
@pytest.mark.parametrize("dtype", K.DTYPES, ids=K.dname)
def test_grad_norm_baseline_within_caps(n, dtype):
    x = K.grad_norm_input(n, dtype, CPU)
    o = K.grad_norm_oracle(x)
    assert o > 0
    assert abs(K.grad_norm_base(x) - o) <= 1e-3 * o


def test_ulp_at():
    assert K.ulp_at(torch.bfloat16, 1.0) == 2.0 ** -7 and K.ulp_at(torch.bfloat16, 3.9) == 2.0 ** -6
    assert K.ulp_at(torch.float16, 0.75) == 2.0 ** -11 and K.ulp_at(torch.float32, 1.5) == 2.0 ** -23
    assert K.ulp_at(torch.float32, 0.0) == 0.0
