"""CPU validation of tests/attention_oracles.py, so that tests/test_attention_rowerr_gpu.py cannot pass
vacuously: for every recipe x {bf16, fp16} x shape x mask mode

* the fp64 oracle equals reference.attention_lse_ref + autograd in fp64 (to 1e-12);
* the unmutated baseline (fp32 opmath, rounding where the kernels round) stays at or below half the
  cap, rho <= 1.5 u, on every output, with and without the inverse RoPE, and inside the lse bound;
* every seeded defect exceeds the cap (3 u) on the output and recipe that CATCHES names, in every case the
  defect applies to, in both dtypes.
"""
import pytest
import torch

from pyrecover_amd.ops import reference as R

from tests import attention_oracles as A

DTYPES = (torch.bfloat16, torch.float16)
SHAPES = [(2, 320, 4, 2, 128), (1, 576, 2, 1, 64), (1, 512, 2, 2, 128), (1, 640, 8, 2, 128), (1, 512, 4, 2, 128)]
MODES = [(True, False), (False, False), (True, True)]  # (causal, packed)
MODE_IDS = ["causal", "full", "packed"]


def _recipes(shape):
    """`stair` needs at least 6 key tiles; (1, 512, 2, 2, 128) is the staircase-only shape."""
    if shape == (1, 512, 2, 2, 128):
        return ("stair5", "stair9")
    return tuple(n for n in A.RECIPES if not n.startswith("stair") or shape[1] >= 6 * A.KT)


def _close(a, b, m=None, tol=1e-12):
    """|a - b| <= 1e-12 of the largest magnitude (m: the abs-oracle's, where the output cancels: column 0 of
    dq in all_negative / all_large is -+198 scale sum(dS), and sum(dS) is 0 in exact math)."""
    return float((a - b).abs().max()) <= tol * max(1.0, float((b if m is None else m).abs().max()))


@pytest.mark.parametrize("dtype", DTYPES, ids=A.dname)
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_oracle_equals_fp64_autograd(shape, mode, dtype):
    causal, packed = mode
    B, S, Hq, Hkv, D = shape
    for name in _recipes(shape):
        c = A.make_case(name, shape, dtype, causal, packed)
        q, k, v = (t.double().requires_grad_() for t in (c.q, c.k, c.v))
        o, lse = R.attention_lse_ref(q, k, v, c.causal, c.scale, c.doc_start)
        o.backward(c.do.double())
        assert _close(c.o, o.detach()) and _close(c.lse, lse.detach()), name
        dq, dk, dv = A.backward_oracle(c.q, c.k, c.v, c.o, c.lse, c.do, c.scale, c.vis)
        assert _close(dq, q.grad, c.m_dq) and _close(dk, k.grad, c.m_dk) and _close(dv, v.grad, c.m_dv), name
        # the inverse RoPE of the oracle is reference.rope_inplace_2d(..., inverse=True)
        want = q.grad.reshape(B * S, Hq * D).clone()
        R.rope_inplace_2d(want, Hq * D, c.tab.double(), D, S, inverse=True, doc_start=c.doc_start)
        assert _close(A.rope_inverse64(dq, c.tab, c.doc_start), want.view(B, S, Hq, D), c.m_dq), name


def _rhos(c, outs, rope):
    o, lse, dq, dk, dv = outs
    return {"o": A.rho(o, c.o, c.m_o)[0], "dq": A.rho(dq, c.dq_rope if rope else c.dq, c.m_dq)[0],
            "dk": A.rho(dk, c.dk_rope if rope else c.dk, c.m_dk)[0], "dv": A.rho(dv, c.dv, c.m_dv)[0]}


@pytest.mark.parametrize("dtype", DTYPES, ids=A.dname)
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_baseline_within_half_cap(shape, mode, dtype):
    causal, packed = mode
    u = A.unit(dtype)
    bad = []
    for name in _recipes(shape):
        c = A.make_case(name, shape, dtype, causal, packed)
        for rope in (False, True):
            outs = A.baseline(c.q, c.k, c.v, c.do, c.scale, c.causal, dtype, c.doc_start,
                              rope_tab=c.tab if rope else None, o_lse=(c.o_in, c.lse_in))
            assert all(bool(torch.isfinite(t).all()) for t in outs), name
            for out, r in _rhos(c, outs, rope).items():
                if not r <= 0.5 * A.cap(dtype, out):
                    bad.append((name, rope, out, round(r / u, 3)))
            lerr = float((outs[1].double() - c.lse).abs().max())
            if not lerr <= c.lse_bound:
                bad.append((name, "lse", lerr, c.lse_bound))
    assert not bad, bad


@pytest.mark.parametrize("dtype", DTYPES, ids=A.dname)
def test_k_prescale_rounding_is_not_row_scaled(dtype):
    """K * scale * log2(e) rounded to the storage dtype (what the 8-wave, ring, pipelined and fused dK/dV
    kernels did before they scaled the fp32 score) shifts a score by up to u * scale * sum|q_d||k_d|, which
    exp turns into a relative error of P: harmless on the flat recipe (scores ~ N(0, 1)), beyond the cap on
    dv where scores are tens of nats. So the cap tells this rounding from the ones it counts."""
    u = A.unit(dtype)
    shape = (1, 512, 4, 2, 128)
    res = {}
    for name in ("flat", "peaked"):
        c = A.make_case(name, shape, dtype, True)
        outs = A.baseline(c.q, c.k, c.v, c.do, c.scale, True, dtype, o_lse=(c.o_in, c.lse_in), k_prescale=True)
        res[name] = _rhos(c, outs, False)
    print("k_prescale rho/u", {n: {o: round(r / u, 2) for o, r in d.items()} for n, d in res.items()})
    assert all(r <= 0.5 * A.cap(dtype, out) for out, r in res["flat"].items()), res["flat"]
    assert res["peaked"]["dv"] > A.cap(dtype, "dv"), res["peaked"]


def test_abs_oracle_rows_are_never_zero():
    """Causal row 0 of dq is exactly 0 in exact math; its error scale is not."""
    c = A.make_case("flat", SHAPES[0], torch.bfloat16, True)
    assert float(c.dq[:, 0].abs().max()) < 1e-12
    for m in (c.m_o, c.m_dq, c.m_dk, c.m_dv):
        assert float(m.reshape(-1, m.shape[-1]).norm(dim=-1).min()) > 0


# mutation -> (recipe, output it must show on, applies(shape, causal, packed)). Measured on the CPU over
# MUT_SHAPES x MODES x DTYPES, smallest rho / u of the named output: lse_shift 5.1 (0.02 / 2^-8),
# delta_zero_tail 60, last_key_zero 78, causal_off_by_one 266, dq_no_scale 49, dk_scale_twice 20,
# gqa_modulo 1500, skip_rescale 223 (peaked) and 2700 (stair9, causal), doc_boundary_ignored 2.7e6.
# `odd_scale` (scale = 1) cannot see the two scale defects and `flat` misses lse_shift and
# delta_zero_tail on full attention (rho 0.3 u and 1.0 u): that is what `peaked` is for.
_always = lambda shape, causal, packed: True  # noqa: E731
CATCHES = {
    "lse_shift": [("peaked", "dv", _always)],
    "delta_zero_tail": [("peaked", "dq", _always)],
    "last_key_zero": [("all_negative", "dv", _always), ("all_negative", "dk", _always)],
    "causal_off_by_one": [("flat", "o", lambda shape, causal, packed: causal)],
    "dq_no_scale": [("peaked", "dq", _always)],
    "dk_scale_twice": [("peaked", "dk", _always)],
    "gqa_modulo": [("flat", "o", lambda shape, causal, packed: shape[3] > 1 and shape[2] > shape[3])],
    "skip_rescale": [("peaked", "o", _always),
                     ("stair9", "o", lambda shape, causal, packed: causal and shape[1] >= 6 * A.KT)],
    "doc_boundary_ignored": [("peaked", "o", lambda shape, causal, packed: packed),
                             ("peaked", "dv", lambda shape, causal, packed: packed)],
}
MUT_SHAPES = [(2, 320, 4, 2, 128), (1, 576, 2, 1, 64)]


def test_every_mutation_is_listed():
    assert set(CATCHES) == set(A.MUTATIONS)
    for entries in CATCHES.values():
        assert all(name in A.RECIPES for name, _, _ in entries)


@pytest.mark.parametrize("dtype", DTYPES, ids=A.dname)
@pytest.mark.parametrize("mutation", A.MUTATIONS)
def test_mutation_exceeds_cap(mutation, dtype):
    """The defect runs through the baseline's own forward and backward (its o and lse feed its
    backward), measured against the unmutated oracle."""
    u = A.unit(dtype)
    seen = 0
    for name, out, applies in CATCHES[mutation]:
        for shape in MUT_SHAPES:
            for causal, packed in MODES:
                if not applies(shape, causal or packed, packed):
                    continue
                c = A.make_case(name, shape, dtype, causal, packed)
                outs = A.baseline(c.q, c.k, c.v, c.do, c.scale, c.causal, dtype, c.doc_start, mutation=mutation)
                r = _rhos(c, outs, False)[out]
                assert r > A.cap(dtype, out), (mutation, name, out, shape, causal, packed, r / u)
                seen += 1
    assert seen > 0
