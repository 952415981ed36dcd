"""Every attention kernel against the fp64 oracle of tests/attention_oracles.py, judged per row:
rho = max_rows |got_r - oracle_r|_2 / |M_r|_2 <= (n_round + 1) u, on adversarial score inputs (a scale
other than 1/sqrt(D), peaked softmax, all-negative / all-large scores, a running max that climbs tile
after tile, non-zero-mean V and dO). Cap, metric, recipes and the seeded defects they catch are
validated on the CPU in tests/test_attention_oracles.py; measured values: profiles/attn_rowerr/README.md.

Shapes (B, S, Hq, Hkv, D), the smallest that reach every loop structure:
  (2, 320, 4, 2, 128)  S untiled (padded to 384): 5 key tiles, so the forward's 3-slot ring wraps; two
                       256-query blocks, the second partial; 4-wave backward kernels
  (1, 576, 2, 1, 64)   9 key tiles, D = 64 (pipelined dK/dV by default), three 256-key blocks, last partial
  (1, 512, 2, 2, 128)  the staircase recipes only
  (1, 640, 8, 2, 128)  the dK/dV query-head split (4 query heads per kv head)
  (1, 512, 4, 2, 128)  S % 256 == 0 at D = 128: the only shapes at which dkdv_kreg 1 / 2 and bwd_fused
                       select a kernel of their own (8-wave blocks; attention.hip attn_bwd_t)
Each backward case runs on oracle-made o (rounded to the storage dtype) and lse (fp32), so a backward
kernel is judged independently of the forward; test_chained_* feed the kernels' own forward output.
Every output must be finite and bit-equal on a second launch.
"""
import functools

import pytest
import torch

from pyrecover_amd import _ext
from tests import attention_oracles as A

pytestmark = pytest.mark.gpu

DTYPES = (torch.bfloat16, torch.float16)
S320, S576, STAIR, S640, S512 = (2, 320, 4, 2, 128), (1, 576, 2, 1, 64), (1, 512, 2, 2, 128), (1, 640, 8, 2, 128), \
    (1, 512, 4, 2, 128)
ALL_SHAPES = [S320, S576, STAIR, S640, S512]
NW8_SHAPES = [STAIR, S512]

# fp32 kernels (attention_f32.hip): rho <= min(4 * measured, 2^-16), `measured` = the largest rho seen on
# the MI355X over FP32_SHAPES x recipes x {causal, full} (profiles/attn_rowerr/README.md)
FP32_MEASURED = {"o": 8.2e-6, "dq": 9.8e-7, "dk": 8.7e-7, "dv": 1.02e-5}
FP32_SHAPES = [S320, S576, S512]


def _recipes(shape):
    if shape == STAIR:
        return ("stair5", "stair9")
    return tuple(n for n in A.RECIPES if not n.startswith("stair") or shape[1] >= 6 * A.KT)


def _select(attn_opts, **sel):
    """Set the kernel selection (everything else at its default) and check that it took."""
    base = dict(fwd_pipe=None, fwd_thr=None, dkdv_impl=None, dq_pipe=None, dkdv_split=None, dkdv_kreg=None,
                bwd_fused=None)
    base.update(sel)
    attn_opts(**base)
    for key, val in sel.items():
        assert _ext._attn_opts[key] == val, (key, _ext._attn_opts[key], val)


class Judge:
    """Collects every figure of a test (printed as ROWERR lines) and fails at the end with all misses."""

    def __init__(self, tag):
        self.tag, self.bad = tag, []

    def row(self, c, what, out, got, want, m, bound):
        u = A.unit(c.dtype) if c.dtype != torch.float32 else A.FP32_CAP
        got = got.detach().cpu()
        if not bool(torch.isfinite(got.float()).all()):
            self.bad.append((c.name, what, out, "not finite"))
            return
        r, i = A.rho(got, want, m)
        print(f"ROWERR {self.tag} {what} {c.name} {A.dname(c.dtype)} {c.shape} causal={c.causal} {out} "
              f"{r / u:.3f} row={i}")
        if not r <= bound:
            self.bad.append((c.name, what, out, f"rho/u={r / u:.3f}", f"cap/u={bound / u:.3f}", f"row={i}"))

    def lse(self, c, what, got):
        got = got.detach().cpu().double()
        fin = torch.isfinite(c.lse)
        err = float((got - c.lse)[fin].abs().max())
        print(f"ROWERR {self.tag} {what} {c.name} {A.dname(c.dtype)} {c.shape} causal={c.causal} lse "
              f"{err:.3e} bound={c.lse_bound:.3e}")
        if not (err <= c.lse_bound and bool(torch.isfinite(got[fin]).all())):
            self.bad.append((c.name, what, "lse", err, c.lse_bound))

    def same(self, c, what, a, b):
        if not all(torch.equal(x, y) for x, y in zip(a, b)):
            self.bad.append((c.name, what, "second launch differs"))

    def done(self):
        assert not self.bad, self.bad


def _bound(c, out):
    if c.dtype == torch.float32:
        return min(4.0 * FP32_MEASURED[out], A.FP32_CAP)
    return A.cap(c.dtype, out)


def _dev(c, cuda):
    return [t.to(cuda) for t in (c.q, c.k, c.v, c.do)]


def _fwd(J, c, cuda, what="fwd"):
    C = _ext.native()
    q, k, v, _ = _dev(c, cuda)
    ds = None if c.doc_start is None else c.doc_start.to(cuda)
    o, lse = C.attn_fwd(q, k, v, c.scale, c.causal, ds)
    o2, lse2 = C.attn_fwd(q, k, v, c.scale, c.causal, ds)
    assert o.dtype == c.dtype and o.shape == c.q.shape and lse.shape == c.lse.shape
    J.same(c, what, (o, lse), (o2, lse2))
    J.row(c, what, "o", o, c.o, c.m_o, _bound(c, "o"))
    J.lse(c, what, lse)
    return o, lse


def _bwd(J, c, cuda, rope, what, o=None, lse=None, want=None):
    """attn_bwd on oracle-made o / lse (default) or on the given ones (chained; `want` = the oracle on them)."""
    C = _ext.native()
    q, k, v, do = _dev(c, cuda)
    o = c.o_in.to(cuda) if o is None else o
    lse = c.lse_in.to(cuda) if lse is None else lse
    tab = c.tab.to(cuda) if rope else None
    ds = None if c.doc_start is None else c.doc_start.to(cuda)
    outs = []
    for _ in range(2):
        d3 = [torch.full_like(t, float("nan")) for t in (q, k, v)]
        C.attn_bwd(q, k, v, o, do, lse, *d3, c.scale, c.causal, tab, 0, ds)
        outs.append(d3)
    what = what + ("+rope" if rope else "")
    J.same(c, what, outs[0], outs[1])
    if want is None:
        want = (c.dq_rope if rope else c.dq, c.dk_rope if rope else c.dk, c.dv)
    for out, got, w, m in zip(("dq", "dk", "dv"), outs[0], want, (c.m_dq, c.m_dk, c.m_dv)):
        J.row(c, what, out, got, w, m, _bound(c, out))


def _chained(J, c, cuda, rope):
    o, lse = _fwd(J, c, cuda, "chain-fwd")
    oc, lc = o.cpu(), lse.cpu()
    dq, dk, dv = A.backward_oracle(c.q, c.k, c.v, oc, lc, c.do, c.scale, c.vis, c.tab if rope else None, c.doc_start)
    _bwd(J, c, cuda, rope, "chain-bwd", o, lse, (dq, dk, dv))


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=A.dname)
@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=str)
@pytest.mark.parametrize("pipe,thr", [(0, 0.0), (0, 8.0), (1, 0.0), (1, 8.0)])
def test_forward(cuda, attn_opts, pipe, thr, shape, causal, dtype):
    """fwd_kernel / fwd_p_kernel, exact and deferred rescale; stair5 crosses fwd_thr = 8 every second
    key tile, stair9 on every tile."""
    _select(attn_opts, fwd_pipe=pipe, fwd_thr=thr)
    J = Judge(f"fwd_pipe={pipe},fwd_thr={thr:g}")
    for name in _recipes(shape):
        _fwd(J, A.make_case(name, shape, dtype, causal), cuda)
    J.done()


BWD_SELECTIONS = [
    ("default", {}, ALL_SHAPES),
    ("dq_pipe=0,dkdv_impl=0,dkdv_kreg=0", dict(dq_pipe=0, dkdv_impl=0, dkdv_kreg=0), ALL_SHAPES),
    ("dq_pipe=1,dkdv_impl=1", dict(dq_pipe=1, dkdv_impl=1, dkdv_split=1), ALL_SHAPES),
    ("dq_pipe=1,dkdv_impl=0,dkdv_kreg=1", dict(dq_pipe=1, dkdv_impl=0, dkdv_kreg=1), NW8_SHAPES),
    ("dq_pipe=0,dkdv_impl=0,dkdv_kreg=2", dict(dq_pipe=0, dkdv_impl=0, dkdv_kreg=2), NW8_SHAPES),
    ("dkdv_impl=1,dkdv_split=2", dict(dq_pipe=0, dkdv_impl=1, dkdv_split=2), [S320, S640, S512]),
    ("dkdv_impl=1,dkdv_split=4", dict(dq_pipe=1, dkdv_impl=1, dkdv_split=4), [S640]),
    ("bwd_fused=1", dict(bwd_fused=1, dkdv_kreg=2, dkdv_impl=0), NW8_SHAPES),
]
BWD_CASES = [pytest.param(sel, shape, id=f"{tag}-{shape}") for tag, sel, shapes in BWD_SELECTIONS for shape in shapes]


def _tag(sel):
    return ",".join(f"{k}={v}" for k, v in sel.items()) or "default"


@pytest.mark.parametrize("dtype", DTYPES, ids=A.dname)
@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("sel,shape", BWD_CASES)
def test_backward(cuda, attn_opts, sel, shape, causal, dtype):
    """dQ (plain / region-pipelined), dK/dV (two-wave with K in LDS / in registers / ring-staged,
    pipelined with the query heads unsplit / split 2 / split 4) and the fused backward, with and without
    the fused inverse RoPE, on oracle-made o and lse.

    This test found the 8-wave two-wave, ring, pipelined and fused dK/dV kernels forming P from
    K * scale * log2(e) rounded to the storage dtype: dv 12-25 u on every recipe with scores of tens of
    nats. They now scale the fp32 score, as the 4-wave and packed kernels always did."""
    _select(attn_opts, **sel)
    J = Judge(_tag(sel))
    for name in _recipes(shape):
        c = A.make_case(name, shape, dtype, causal)
        for rope in (False, True):
            _bwd(J, c, cuda, rope, "bwd")
    J.done()


@pytest.mark.parametrize("dtype", DTYPES, ids=A.dname)
@pytest.mark.parametrize("sel,shape", [pytest.param(sel, shapes[-1], id=tag) for tag, sel, shapes in BWD_SELECTIONS])
def test_chained_backward(cuda, attn_opts, sel, shape, dtype):
    """One case per backward kernel selection on the kernels' own forward output (peaked, causal, RoPE)."""
    _select(attn_opts, **sel)
    J = Judge(_tag(sel))
    _chained(J, A.make_case("peaked", shape, dtype, True), cuda, rope=True)
    J.done()


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("shape", FP32_SHAPES, ids=str)
def test_fp32_kernels(cuda, shape, causal):
    """attention_f32.hip on every recipe that fits fp32 (attention_oracles.fits_fp32: scores below 44
    nats; that leaves out peaked, stair9, all_negative and all_large); a causal case also runs chained."""
    J = Judge("fp32")
    ran = []
    for name in _recipes(shape):
        c = A.make_case(name, shape, torch.float32, causal)
        if not A.fits_fp32(c.smax):
            continue
        ran.append(name)
        _fwd(J, c, cuda)
        _bwd(J, c, cuda, False, "bwd")
    assert {"flat", "peaked_rsqrt", "spike_rows", "odd_scale"} <= set(ran), ran
    if causal:
        c = A.make_case("peaked_rsqrt", shape, torch.float32, True)
        o, lse = _fwd(J, c, cuda, "chain-fwd")
        want = A.backward_oracle(c.q, c.k, c.v, o.cpu(), lse.cpu(), c.do, c.scale, c.vis)
        _bwd(J, c, cuda, False, "chain-bwd", o, lse, want)
    J.done()


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=A.dname)
@pytest.mark.parametrize("shape", [S320, S576], ids=str)
def test_packed_kernels(cuda, shape, dtype):
    """attention_docs.hip with document boundaries inside a key tile (37), on a tile edge (128) and
    one-token documents (200, 201, 202), and a last document of one token in the other sequences."""
    J = Judge("packed")
    for name in ("peaked", "spike_rows"):
        c = A.make_case(name, shape, dtype, True, True)
        _fwd(J, c, cuda)
        for rope in (False, True):
            _bwd(J, c, cuda, rope, "bwd")
    _chained(J, A.make_case("peaked", shape, dtype, True, True), cuda, rope=True)
    J.done()


# ------------------------------------------------------------------------------------------------
KV_LEN = (1, 255, 256, 257, 3 * 256 + 17)


@functools.lru_cache(maxsize=None)
def _decode_case(name, D, dtype):
    """One ragged batch: a single key, one below / at / one above the 256-key chunk, and three chunks
    plus 17; GQA 4 / 2. The query is the recipe's first row, the caches are its K and V."""
    B, cap, Hq, Hkv = len(KV_LEN), max(KV_LEN) + 7, 4, 2
    q, k, v, _, scale = A.recipe(name, B, cap, Hq, Hkv, D, dtype, causal=False)
    c = A.Case()
    c.name, c.shape, c.dtype, c.causal, c.scale = name, (B, cap, Hq, Hkv, D), dtype, False, scale
    c.q, c.k, c.v = q[:, :1].contiguous(), k, v
    c.kv_len = torch.tensor(KV_LEN, dtype=torch.int32)
    c.vis = A.visibility(B, 1, cap, False, kv_len=c.kv_len)
    c.o, c.lse = A.forward_oracle(c.q, k, v, scale, c.vis)
    (c.m_o,) = A.abs_oracle(c.q, k, v, None, c.lse, None, scale, c.vis, dtype)
    c.lse_bound, c.smax = A.lse_bound(c.q, k, scale, c.vis, c.lse)
    return c


@pytest.mark.parametrize("dtype", DTYPES, ids=A.dname)
@pytest.mark.parametrize("D", [64, 128])
def test_decode(cuda, D, dtype):
    """attn_decode (attention_decode.hip): P and the chunk partials stay fp32, so o has one rounding."""
    C = _ext.native()
    assert C.attn_decode_chunk() == 256  # KV_LEN straddles the chunk
    J = Judge("decode")
    for name in ("peaked", "all_negative", "all_large", "stair5", "stair9"):
        c = _decode_case(name, D, dtype)
        q, k, v, n = c.q[:, 0].to(cuda), c.k.to(cuda), c.v.to(cuda), c.kv_len.to(cuda)
        o, lse = C.attn_decode(q, k, v, n, c.scale)
        o2, lse2 = C.attn_decode(q, k, v, n, c.scale)
        J.same(c, "decode", (o, lse), (o2, lse2))
        J.row(c, "decode", "o", o[:, None], c.o, c.m_o, A.cap(dtype, "decode_o"))
        J.lse(c, "decode", lse[:, :, None])
    J.done()
