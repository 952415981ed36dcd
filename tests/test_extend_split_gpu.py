"""The key-split arm of attn_extend (csrc/kernels/attention_extend_split.hip, chunks of XC = attn_extend_chunk()
keys) against the torch oracle and its bit contract, the plan that chooses it (attn_extend_plan.h) and the model
level. Inputs, reference and bounds are test_extend_gpu.py's: the split changes only the order of fp32 sums."""
import math

import pytest
import torch

from pyrecover_amd import _ext
from pyrecover_amd import inference as inf
from pyrecover_amd.config import get_preset
from pyrecover_amd.models.llama import Transformer
from pyrecover_amd.ops import reference as R
from tests.test_extend_gpu import CONFIGS, LSE_TOL, O_TOL, _inputs, _lens, _ref_forward

pytestmark = pytest.mark.gpu


def _xc_bases():
    """XC and, for cap = 2 * XC + 150: an empty cache (chunk 0 only), rows of one tile with different last chunks,
    a chunk that holds one visible key (base XC, row 0), a partial third chunk."""
    XC = _ext.native().attn_extend_chunk()
    return XC, [0, 1, XC - 3, XC, 2 * XC + 100]


def _check(q, k, v, n, D):
    scale = 1 / math.sqrt(D)
    o, lse = _ext.native().attn_extend(q, k, v, n, scale, split=1)
    o_ref, lse_ref = R.attention_extend_ref(q.float(), k.float(), v.float(), n, scale)
    assert o.dtype == q.dtype and lse.dtype == torch.float32 and o.shape == q.shape and lse.shape == q.shape[:3]
    assert torch.isfinite(o).all() and torch.isfinite(lse).all()
    eo, el = (o.float() - o_ref).abs().max().item(), (lse - lse_ref).abs().max().item()
    print(f"|o - o_ref| = {eo:.3e}, |lse - lse_ref| = {el:.3e}")
    assert eo < O_TOL and el < LSE_TOL
    return o, lse


@pytest.mark.parametrize("dtype,D", [(torch.bfloat16, 128), (torch.float16, 128), (torch.bfloat16, 64)])
@pytest.mark.parametrize("T,Hq,Hkv", [(T, hq, hkv) for T in (5, 33, 135) for hq, hkv in ((2, 2), (8, 1))] + [(8, 4, 1)])
def test_attn_extend_split_vs_reference(cuda, dtype, D, T, Hq, Hkv):
    """R = T * G = 5, 40 (4 and 2 waves per sub-tile), 33, 264, 135, 1080 (1 wave; ragged row tiles) and an exactly
    full 32 rows (T 8, G 4), over three chunks."""
    XC, base = _xc_bases()
    q, k, v = _inputs(cuda, len(base), T, 2 * XC + 150, Hq, Hkv, D, dtype)
    _check(q, k, v, _lens(cuda, base), D)


@pytest.mark.parametrize("D,Hq,Hkv", [(128, 2, 2), (64, 8, 1)])
@pytest.mark.parametrize("where", ["last", "chunk0"])
def test_attn_extend_split_combine_weights(cuda, D, Hq, Hkv, where):
    """One huge q.k for head 0 of the last row (test_attn_extend_late_score_spike's), at its last visible key (the
    combine must scale the earlier chunks down) or at key 3 (the later chunks must add almost nothing): that head
    is all but the spike's value row."""
    XC = _xc_bases()[0]
    T, base = 135, XC + 20
    q, k, v = _inputs(cuda, 1, T, 2 * XC + 150, Hq, Hkv, D, torch.bfloat16, seed=3)
    at = base + T - 1 if where == "last" else 3
    q[0, T - 1, 0] = 4.0
    k[0, at, 0] = 4.0
    o, _ = _check(q, k, v, _lens(cuda, [base]), D)
    assert (o[0, T - 1, 0].float() - v[0, at, 0].float()).abs().max().item() < O_TOL


def test_attn_extend_split_bits(cuda):
    """Equal bits: run to run, contiguous q against the strided view, a NaN / Inf tail beyond kv_len + T against
    a zero tail, the same contents in a cache one chunk and a bit longer, each sequence alone against the batch."""
    C = _ext.native()
    XC, base = _xc_bases()
    D, Hq, Hkv, T, cap = 128, 8, 2, 33, 2 * XC + 150
    scale = 1 / math.sqrt(D)
    q, k, v = _inputs(cuda, len(base), T, cap, Hq, Hkv, D, torch.bfloat16, seed=1)
    n = _lens(cuda, base)

    def same(q_, k_, v_, n_, o_, lse_):
        o2, lse2 = C.attn_extend(q_, k_, v_, n_, scale, split=1)
        return torch.equal(o2, o_) and torch.equal(lse2, lse_)

    o, lse = C.attn_extend(q, k, v, n, scale, split=1)
    assert same(q, k, v, n, o, lse)
    assert same(q.contiguous(), k, v, n, o, lse)
    kp, vp, kz, vz = k.clone(), v.clone(), k.clone(), v.clone()
    for b, L in enumerate(base):
        kz[b, L + T:], vz[b, L + T:] = 0, 0
        kp[b, L + T:L + T + 5], vp[b, L + T:L + T + 5] = float("nan"), float("inf")
        kp[b, L + T + 5:], vp[b, L + T + 5:] = float("-inf"), float("nan")
    assert same(q, kp, vp, n, o, lse) and same(q, kz, vz, n, o, lse)
    big = cap + XC + 64
    kb, vb = (torch.randn(len(base), big, Hkv, D, device=cuda).bfloat16() for _ in range(2))
    kb[:, :cap], vb[:, :cap] = k, v
    assert same(q, kb, vb, n, o, lse)
    for b in range(len(base)):
        assert same(q[b:b + 1], k[b:b + 1], v[b:b + 1], n[b:b + 1], o[b:b + 1], lse[b:b + 1]), b


def test_attn_extend_split_clamps(cuda):
    """test_attn_extend_clamps on the split: kv_len -3 and cap + 5 behave as 0 and cap, rows past the capacity see
    the whole cache, everything is finite and the caches are not written."""
    C = _ext.native()
    D, Hq, Hkv, T, cap, scale = 64, 4, 2, 33, 2 * _xc_bases()[0] + 150, 0.125
    q, k, v = _inputs(cuda, 4, T, cap, Hq, Hkv, D, torch.float16, seed=2)
    k0, v0 = k.clone(), v.clone()
    o, lse = C.attn_extend(q, k, v, _lens(cuda, [-3, cap + 5, cap - 10, cap - T]), scale, split=1)
    oc, lc = C.attn_extend(q, k, v, _lens(cuda, [0, cap, cap - 10, cap - T]), scale, split=1)
    assert torch.equal(o, oc) and torch.equal(lse, lc)
    assert torch.isfinite(o).all() and torch.isfinite(lse).all()
    assert torch.equal(k, k0) and torch.equal(v, v0)
    _check(q, k, v, _lens(cuda, [-3, cap + 5, cap - 10, cap - T]), D)


def test_attn_extend_plan(cuda):
    """Pinned rows of the plan (auto splits iff ceil(cap / XC) >= 4 and 2 * blocks1 <= CUs), the rejected split
    value, and auto = single pass in bits at the shape of test_attn_extend_bits."""
    C = _ext.native()
    XC = C.attn_extend_chunk()
    NC = 8192 // XC
    assert XC % 256 == 0 and torch.cuda.get_device_properties(cuda).multi_processor_count == 256
    assert C.attn_extend_plan(1, 8, 32, 8, 128, 8192) == {"split": True, "ws_waves": 4, "chunks": NC, "blocks": 8 * NC,
                                                          "ws_floats": 8 * 32 * NC * 130}
    p = C.attn_extend_plan(4, 2048, 32, 32, 128, 2048)
    assert not p["split"] and p["blocks"] == 16 * 32 * 4 and p["ws_floats"] == 0
    for cap in (400, 864):
        p = C.attn_extend_plan(5, 33, 8, 2, 128, cap)
        assert not p["split"] and p["blocks"] == 2 * 2 * 5
    # 2048 rows per kv head: blocks1 = 16 * 8 = 128, half of the CUs, so the rule splits
    p = C.attn_extend_plan(1, 512, 32, 8, 128, 8192)
    assert p["split"] and p["ws_waves"] == 1 and p["blocks"] == 128 * (8192 // XC)
    assert not C.attn_extend_plan(2, 512, 32, 8, 128, 8192)["split"]
    scale = 1 / math.sqrt(128)
    q, k, v = _inputs(cuda, 5, 33, 400, 8, 2, 128, torch.bfloat16, seed=1)
    n = _lens(cuda, [0, 1, 63, 64, 200])
    with pytest.raises(RuntimeError, match="split"):
        C.attn_extend(q, k, v, n, scale, split=2)
    (oa, la), (o0, l0) = C.attn_extend(q, k, v, n, scale, split=-1), C.attn_extend(q, k, v, n, scale, split=0)
    assert torch.equal(oa, o0) and torch.equal(la, l0)


def test_extend_split_logits_vs_fp32_model(cuda):
    """head_dim 128, GQA 4:1, a cache of 4 * XC + 64 rows: prefill 4 * XC - 24 tokens, extend 16 (return_all), a
    ragged extend (n_new = [8, 3]) up to the chunk boundary and one of 4 tokens across it, all on the key split by
    plan. The rule of test_extend_logits_vs_fp32_model on rows P - 1 .. end: e_ext <= 2 * e_full + 1e-3.

    Measured on MI355X (XC 512): e_full 1.001e-2, e_ext 1.001e-2 (both are the rounding of the same bf16 logit)."""
    C = _ext.native()
    XC = C.attn_extend_chunk()
    S, B, P, E, N, n_new = 4 * XC + 64, 2, 4 * XC - 24, 16, 4, [8, 3]
    for T in (E, max(n_new), N):
        assert C.attn_extend_plan(B, T, 4, 1, 128, S)["split"], T
    torch.manual_seed(0)
    cfg = get_preset(CONFIGS[1][0], seq_len=S, **CONFIGS[1][1])
    m32 = Transformer(cfg).to(cuda).eval()
    m = Transformer(cfg).to(cuda)
    m.load_state_dict(m32.state_dict())
    m = m.bfloat16().eval()
    m32.load_state_dict(m.state_dict())  # the same (bf16-representable) weights in fp32
    tok = torch.randint(0, cfg.vocab_size, (B, P + E + max(n_new) + N), device=cuda)
    L = [P + E + n + N for n in n_new]
    with torch.no_grad():
        ref_all, full_all = _ref_forward(m32, tok), m(tok).float()
        cache = inf.KVCache(cfg, B, S, torch.bfloat16, cuda)
        first = inf.prefill(m, tok[:, :P], torch.full((B,), P, device=cuda), cache)
        ext = inf.extend(m, tok[:, P:P + E], torch.full((B,), E, device=cuda), cache, return_all=True)
        rag_tok = torch.zeros(B, max(n_new), dtype=torch.long, device=cuda)
        for b in range(B):
            rag_tok[b, :n_new[b]] = tok[b, P + E:P + E + n_new[b]]
        rag = inf.extend(m, rag_tok, torch.tensor(n_new, device=cuda), cache, return_all=True)
        assert cache.kv_len.tolist() == [P + E + n for n in n_new]
        last_tok = torch.stack([tok[b, P + E + n_new[b]:L[b]] for b in range(B)])
        last = inf.extend(m, last_tok, torch.full((B,), N, device=cuda), cache, return_all=True)
    e_full = e_ext = 0.0
    for b in range(B):
        got = torch.cat([first[b:b + 1], ext[b], rag[b, :n_new[b]], last[b]]).float()
        ref = ref_all[b, P - 1:L[b]]
        assert got.shape == ref.shape
        e_full = max(e_full, (full_all[b, P - 1:L[b]] - ref).abs().max().item())
        e_ext = max(e_ext, (got - ref).abs().max().item())
    print(f"e_full = {e_full:.3e}, e_ext = {e_ext:.3e}")
    assert e_ext <= 2 * e_full + 1e-3
