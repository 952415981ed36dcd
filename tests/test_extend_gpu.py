"""Multi-token KV-cache append on the GPU: attn_extend (csrc/kernels/attention_extend.hip) and the T-token
rope_append against the torch oracle and against their bit-reproducibility contract, and the model-level
extend / chunked-prefill paths against the fp32 plain-torch model."""
import math
import warnings

import pytest
import torch

from pyrecover_amd import _ext
from pyrecover_amd import inference as inf
from pyrecover_amd.config import get_preset
from pyrecover_amd.models.llama import Transformer
from pyrecover_amd.ops import reference as R

pytestmark = pytest.mark.gpu

# bounds of test_kernels_gpu.py::test_attention_fwd
O_TOL, LSE_TOL = 2e-2, 1e-3

CAP = 400
KV_LEN = [0, 1, 63, 64, 200]  # an empty cache, and both sides of a 64-key tile boundary


def _inputs(cuda, B, T, cap, Hq, Hkv, D, dtype, seed=0):
    """Standard normal q and caches, as test_generate_gpu.py::_inputs makes them. q is the [B, T, Hq, D] view of
    the q columns of a fused QKV activation [B * T, (Hq + 2 Hkv) D]: token rows strided, as ``extend`` passes it."""
    torch.manual_seed(seed)
    qkv = torch.randn(B * T, (Hq + 2 * Hkv) * D, device=cuda).to(dtype)
    q = qkv[:, :Hq * D].view(B, T, Hq, D)
    k = torch.randn(B, cap, Hkv, D, device=cuda).to(dtype)
    v = torch.randn(B, cap, Hkv, D, device=cuda).to(dtype)
    return q, k, v


def _lens(cuda, lens):
    return torch.tensor(lens, device=cuda, dtype=torch.int32)


def _check(q, k, v, n, D):
    C = _ext.native()
    scale = 1 / math.sqrt(D)
    o, lse = C.attn_extend(q, k, v, n, scale)
    o_ref, lse_ref = R.attention_extend_ref(q.float(), k.float(), v.float(), n, scale)
    assert o.dtype == q.dtype and lse.dtype == torch.float32
    assert o.shape == q.shape and lse.shape == q.shape[:3]
    assert torch.isfinite(o).all() and torch.isfinite(lse).all()
    eo = (o.float() - o_ref).abs().max().item()
    el = (lse - lse_ref).abs().max().item()
    print(f"|o - o_ref| = {eo:.3e}, |lse - lse_ref| = {el:.3e}")
    assert eo < O_TOL and el < LSE_TOL
    return o, lse


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Hq,Hkv", [(2, 2), (4, 1), (8, 1)])
@pytest.mark.parametrize("T", [1, 5, 33, 135])
def test_attn_extend_vs_reference(cuda, dtype, D, Hq, Hkv, T):
    """T x G rows per (sequence, kv head): a partial wave (1 .. 40 rows), one block and four rows (33 x 4),
    several row tiles with a ragged last one (up to 135 x 8 = 1080 rows), bases on both sides of a key-tile
    boundary and an empty cache. Exactly full waves and blocks: test_attn_extend_full_waves."""
    q, k, v = _inputs(cuda, len(KV_LEN), T, CAP, Hq, Hkv, D, dtype)
    _check(q, k, v, _lens(cuda, KV_LEN), D)


@pytest.mark.parametrize("T,Hq,Hkv", [(8, 4, 1), (16, 8, 1), (32, 2, 2), (128, 2, 2)])
def test_attn_extend_full_waves(cuda, T, Hq, Hkv):
    """T x G = 32 (one exactly full wave), 128 (one exactly full block), 32 and 128 at G = 1."""
    q, k, v = _inputs(cuda, len(KV_LEN), T, CAP, Hq, Hkv, 128, torch.bfloat16, seed=5)
    _check(q, k, v, _lens(cuda, KV_LEN), 128)


@pytest.mark.parametrize("D,Hq,Hkv", [(128, 2, 2), (64, 8, 1)])
def test_attn_extend_late_score_spike(cuda, D, Hq, Hkv):
    """One huge q.k at the last visible key of the last row (as test_attn_decode_late_score_spike): everything
    accumulated over the earlier tiles must be rescaled by it."""
    T, base = 135, 200
    q, k, v = _inputs(cuda, 1, T, CAP, Hq, Hkv, D, torch.bfloat16, seed=3)
    q[0, T - 1, 0] = 4.0
    k[0, base + T - 1, 0] = 4.0
    o, _ = _check(q, k, v, _lens(cuda, [base]), D)
    # head 0 of the last row is all but that one value row
    assert (o[0, T - 1, 0].float() - v[0, base + T - 1, 0].float()).abs().max().item() < O_TOL


def test_attn_extend_bits(cuda):
    """Run-to-run bits; a NaN / Inf cache tail beyond kv_len + T against a zero tail; a larger cap with the
    same contents; a contiguous q against the strided view."""
    C = _ext.native()
    D, Hq, Hkv, T = 128, 8, 2, 33
    scale = 1 / math.sqrt(D)
    base = [0, 1, 63, 64, 200]
    q, k, v = _inputs(cuda, len(base), T, CAP, Hq, Hkv, D, torch.bfloat16, seed=1)
    n = _lens(cuda, base)
    o, lse = C.attn_extend(q, k, v, n, scale)
    o2, lse2 = C.attn_extend(q, k, v, n, scale)
    assert torch.equal(o, o2) and torch.equal(lse, lse2)
    oc, lc = C.attn_extend(q.contiguous(), k, v, n, scale)
    assert torch.equal(o, oc) and torch.equal(lse, lc)
    # poisoned tails against zero tails
    kp, vp, kz, vz = k.clone(), v.clone(), k.clone(), v.clone()
    for b, L in enumerate(base):
        kz[b, L + T:], vz[b, L + T:] = 0, 0
        kp[b, L + T:L + T + 5], vp[b, L + T:L + T + 5] = float("nan"), float("inf")
        kp[b, L + T + 5:], vp[b, L + T + 5:] = float("-inf"), float("nan")
    op, lp = C.attn_extend(q, kp, vp, n, scale)
    oz, lz = C.attn_extend(q, kz, vz, n, scale)
    assert torch.equal(op, oz) and torch.equal(lp, lz) and torch.equal(op, o) and torch.equal(lp, lse)
    # the same contents in a larger cache
    big = 2 * CAP + 64
    kb, vb = (torch.randn(len(base), big, Hkv, D, device=cuda).bfloat16() for _ in range(2))
    kb[:, :CAP], vb[:, :CAP] = k, v
    ob, lb = C.attn_extend(q, kb, vb, n, scale)
    assert torch.equal(ob, o) and torch.equal(lb, lse)


def test_attn_extend_clamps(cuda):
    """kv_len -3 and cap + 5 behave as 0 and cap; with kv_len + T > cap the rows past the capacity see keys
    0 .. cap - 1 (the reference's clamp), everything is finite and the caches are not written."""
    C = _ext.native()
    D, Hq, Hkv, T, cap = 64, 4, 2, 33, 300
    scale = 1 / math.sqrt(D)
    q, k, v = _inputs(cuda, 4, T, cap, Hq, Hkv, D, torch.float16, seed=2)
    k0, v0 = k.clone(), v.clone()
    o, lse = C.attn_extend(q, k, v, _lens(cuda, [-3, cap + 5, cap - 10, cap - T]), scale)
    oc, lc = C.attn_extend(q, k, v, _lens(cuda, [0, cap, cap - 10, cap - T]), scale)
    assert torch.equal(o, oc) and torch.equal(lse, lc)
    assert torch.isfinite(o).all() and torch.isfinite(lse).all()
    assert torch.equal(k, k0) and torch.equal(v, v0)
    _check(q, k, v, _lens(cuda, [-3, cap + 5, cap - 10, cap - T]), D)
    # a row at or beyond the capacity is a decode query over the whole cache
    od, _ = R.attention_decode_ref(q[1:3, -1].float(), k[1:3].float(), v[1:3].float(), _lens(cuda, [cap, cap]), scale)
    assert (o[1:3, -1].float() - od).abs().max().item() < O_TOL


# ---------------------------------------------------------------------------------------
def _rope_case(cuda, B, T, cap, Hq, Hkv, D, dtype, seed=0):
    tab = R.rope_table(R.precompute_freqs_cis(D, cap + T)).to(cuda)  # rope_ reads base + T rows
    torch.manual_seed(seed)
    qkv = torch.randn(B * T, (Hq + 2 * Hkv) * D, device=cuda).to(dtype)
    kc = torch.randn(B, cap, Hkv, D, device=cuda).to(dtype)
    vc = torch.randn_like(kc)
    return tab, qkv, kc, vc


def _rope_check(cuda, tab, qkv, kc, vc, base, T, Hq, Hkv, D):
    """rope_append_ at ``base`` against rope_ on the same rows; returns after asserting q bits, the stored rows
    and that every other cache row is untouched."""
    C = _ext.native()
    B, cap = kc.shape[0], kc.shape[1]
    nq, nk = Hq * D, Hkv * D
    kc0, vc0 = kc.clone(), vc.clone()
    want = qkv.clone()
    for b in range(B):
        p0 = min(max(base[b], 0), cap)
        fit = max(min(T, cap - p0), 0)  # rows with a position below the capacity
        if T == 1:
            C.rope_(want[b:b + 1], nq + nk, tab, D, 1, min(p0, cap - 1), False, None)
        else:
            if fit:
                C.rope_(want[b * T:b * T + fit], nq + nk, tab, D, fit, p0, False, None)
            for t in range(fit, T):  # past the capacity: table row cap - 1
                C.rope_(want[b * T + t:b * T + t + 1], nq + nk, tab, D, 1, cap - 1, False, None)
    got = qkv.clone()
    C.rope_append_(got, tab, _lens(cuda, base), kc, vc)
    assert torch.equal(got[:, :nq], want[:, :nq])
    assert torch.equal(got[:, nq:], qkv[:, nq:])  # k and v columns of the activation stay
    for b in range(B):
        p0 = min(max(base[b], 0), cap)
        for t in range(T):
            p = p0 + t
            if T == 1:
                p = min(p, cap - 1)
            if p < cap:
                assert torch.equal(kc[b, p].reshape(-1), want[b * T + t, nq:nq + nk]), (b, t)
                assert torch.equal(vc[b, p].reshape(-1), qkv[b * T + t, nq + nk:]), (b, t)
                kc0[b, p], vc0[b, p] = kc[b, p], vc[b, p]
    assert torch.equal(kc, kc0) and torch.equal(vc, vc0)  # nothing else written


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("D,Hq,Hkv", [(64, 4, 2), (128, 8, 1)])
def test_rope_append_multi_token_bits(cuda, dtype, D, Hq, Hkv):
    """q and the cache rows bit-equal to rope_ at positions kv_len[b] + t, v an exact copy, every other cache
    row untouched: ragged bases including 0 and cap - T, then bases that run past the capacity (nothing stored
    there, q rotated with table row cap - 1), then the single-token call's clamp to cap - 1."""
    cap, B, T = 40, 4, 5
    tab, qkv, kc, vc = _rope_case(cuda, B, T, cap, Hq, Hkv, D, dtype)
    _rope_check(cuda, tab, qkv, kc, vc, [0, cap - T, 7, 20], T, Hq, Hkv, D)
    _rope_check(cuda, tab, qkv, kc, vc, [cap - 2, cap + 9, -2, cap - T + 1], T, Hq, Hkv, D)
    tab, qkv, kc, vc = _rope_case(cuda, B, 1, cap, Hq, Hkv, D, dtype, seed=1)
    _rope_check(cuda, tab, qkv, kc, vc, [0, cap - 1, 7, 20], 1, Hq, Hkv, D)
    _rope_check(cuda, tab, qkv, kc, vc, [-2, cap + 9, cap, 20], 1, Hq, Hkv, D)


def test_rope_append_multi_token_grid_stride(cuda):
    """More 8-column items (4 x 1024 x 160) than the capped grid has lanes: the loop's second pass."""
    cap, B, T, Hq, Hkv, D = 1100, 4, 1024, 8, 1, 128
    tab, qkv, kc, vc = _rope_case(cuda, B, T, cap, Hq, Hkv, D, torch.bfloat16, seed=2)
    C = _ext.native()
    nq, nk = Hq * D, Hkv * D
    base = [0, 76, 13, 50]
    want = qkv.clone()
    for b in range(B):
        C.rope_(want[b * T:(b + 1) * T], nq + nk, tab, D, T, base[b], False, None)
    kc0, vc0 = kc.clone(), vc.clone()
    got = qkv.clone()
    C.rope_append_(got, tab, _lens(cuda, base), kc, vc)
    assert torch.equal(got[:, :nq], want[:, :nq]) and torch.equal(got[:, nq:], qkv[:, nq:])
    for b in range(B):
        rows = slice(base[b], base[b] + T)
        assert torch.equal(kc[b, rows].reshape(T, nk), want[b * T:(b + 1) * T, nq:nq + nk])
        assert torch.equal(vc[b, rows].reshape(T, nk), qkv[b * T:(b + 1) * T, nq + nk:])
        kc0[b, rows], vc0[b, rows] = kc[b, rows], vc[b, rows]
    assert torch.equal(kc, kc0) and torch.equal(vc, vc0)


def test_extend_bindings_reject_bad_arguments(cuda):
    C = _ext.native()
    D, Hq, Hkv, cap, T = 64, 4, 2, 32, 3
    q, k, v = _inputs(cuda, 2, T, cap, Hq, Hkv, D, torch.bfloat16)
    n = _lens(cuda, [3, 4])
    tab = R.rope_table(R.precompute_freqs_cis(D, cap)).to(cuda)
    qkv = torch.randn(2 * T, (Hq + 2 * Hkv) * D, device=cuda).bfloat16()
    C.attn_extend(q, k, v, n, 0.125)  # the good calls
    C.rope_append_(qkv.clone(), tab, n, k.clone(), v.clone())
    with pytest.raises(RuntimeError, match="bf16 or fp16"):
        C.attn_extend(q.float(), k.float(), v.float(), n, 0.125)
    with pytest.raises(RuntimeError, match="dtype"):
        C.attn_extend(q, k.half(), v, n, 0.125)
    with pytest.raises(RuntimeError, match="must be on"):
        C.attn_extend(q, k.cpu(), v, n, 0.125)
    with pytest.raises(RuntimeError, match="must be on"):
        C.attn_extend(q, k, v, n.cpu(), 0.125)
    with pytest.raises(RuntimeError, match="int32"):
        C.attn_extend(q, k, v, n.long(), 0.125)
    q96, k96, v96 = _inputs(cuda, 2, T, cap, Hq, Hkv, 96, torch.bfloat16)
    with pytest.raises(RuntimeError, match="head_dim"):
        C.attn_extend(q96, k96, v96, n, 0.1)
    kt = torch.randn(2, Hkv, cap, D, device=cuda).bfloat16().transpose(1, 2)  # [B, cap, Hkv, D], not contiguous
    with pytest.raises(RuntimeError, match="contiguous"):
        C.attn_extend(q, kt, v, n, 0.125)
    with pytest.raises(RuntimeError, match=r"q must be \[B, T, Hq, D\]"):
        C.attn_extend(q[:, 0], k, v, n, 0.125)
    with pytest.raises(RuntimeError, match="k_cache must be"):
        C.attn_extend(q[:1], k, v, n, 0.125)
    with pytest.raises(RuntimeError, match="multiple of n_kv_heads"):
        C.attn_extend(q[:, :, :3].contiguous(), k, v, n, 0.125)
    with pytest.raises(RuntimeError, match="contiguous"):
        C.rope_append_(qkv.clone(), tab, n, kt, v)
    with pytest.raises(RuntimeError, match="T rows for each"):
        C.rope_append_(qkv[:5].clone(), tab, n, k, v)
    with pytest.raises(RuntimeError, match="qkv must be"):
        C.rope_append_(qkv[:, :-D].contiguous(), tab, n, k, v)


# ---------------------------------------------------------------------------------------
def _ref_forward(m, tok):
    """The reference model as plain torch modules (no fused op), in the dtype of ``m``."""
    B, S = tok.shape
    h = torch.nn.functional.embedding(tok, m.tok_embeddings.weight)
    for L in m.layers.values():
        at = L.attention
        x = L.attention_norm(h)
        q = (x @ at.wq.weight.t()).view(B, S, at.n_heads, at.head_dim)
        k = (x @ at.wk.weight.t()).view(B, S, at.n_kv_heads, at.head_dim)
        v = (x @ at.wv.weight.t()).view(B, S, at.n_kv_heads, at.head_dim)
        q, k = R.apply_rotary_emb_ref(q, k, m.freqs_cis)
        o = R.attention_ref(q, k, v, True).reshape(B, S, -1)
        h = h + o @ at.wo.weight.t()
        x = L.ffn_norm(h)
        ff = L.feed_forward
        h = h + R.swiglu_ref(x @ ff.w1.weight.t(), x @ ff.w3.weight.t()) @ ff.w2.weight.t()
    return m.norm(h) @ m.output.weight.t()


CONFIGS = [
    ("llama-tiny", {}),  # head_dim 64, GQA 2:1
    ("llama-tiny", {"dim": 512, "n_heads": 4, "n_kv_heads": 1}),  # 2 layers, head_dim 128, GQA 4:1
]


def _models(cuda, preset, over):
    torch.manual_seed(0)
    cfg = get_preset(preset, seq_len=128, **over)
    m32 = Transformer(cfg).to(cuda).eval()
    m = Transformer(cfg).to(cuda)
    m.load_state_dict(m32.state_dict())
    m = m.bfloat16().eval()
    m32.load_state_dict(m.state_dict())  # the same (bf16-representable) weights in fp32
    return cfg, m32, m


@pytest.mark.parametrize("preset,over", CONFIGS)
def test_extend_logits_vs_fp32_model(cuda, preset, over):
    """Teacher-forced, bf16: 40-token prefill, a 16-token extend, a ragged extend (n_new = [8, 3]) and 4 decode
    steps, every row's logits kept (return_all). With e_full / e_ext the max abs error of the HIP full-forward /
    this path's logits against the fp32 plain-torch model on the same rows (39 .. end of each sequence), require
    e_ext <= 2 * e_full + 1e-3 (different GEMM shapes and summation orders at identical rounding points; the
    floor is for near-zero logits): the rule of test_decode_logits_vs_fp32_model.

    Measured on MI355X: llama-tiny e_full 1.077e-2, e_ext 1.077e-2; head_dim-128 GQA 4:1 e_full 1.100e-2,
    e_ext 1.100e-2 (both are the rounding of the same bf16 logit)."""
    cfg, m32, m = _models(cuda, preset, over)
    B, P, E, N = 2, 40, 16, 4
    n_new = [8, 3]
    tok = torch.randint(0, cfg.vocab_size, (B, P + E + max(n_new) + N), device=cuda)
    L = [P + E + n + N for n in n_new]  # each sequence's own stream is tok[b, :L[b]]; causal: the rest is inert
    with torch.no_grad():
        ref_all, full_all = _ref_forward(m32, tok), m(tok).float()
        ref = [ref_all[b, P - 1:L[b]] for b in range(B)]
        full = [full_all[b, P - 1:L[b]] for b in range(B)]
        cache = inf.KVCache(cfg, B, max(L), torch.bfloat16, cuda)
        first = inf.prefill(m, tok[:, :P], torch.full((B,), P, device=cuda), cache)
        ext = inf.extend(m, tok[:, P:P + E], torch.full((B,), E, device=cuda), cache, return_all=True)
        assert cache.kv_len.tolist() == [P + E] * B
        rag_tok = torch.zeros(B, max(n_new), dtype=torch.long, device=cuda)
        for b in range(B):
            rag_tok[b, :n_new[b]] = tok[b, P + E:P + E + n_new[b]]
        rag = inf.extend(m, rag_tok, torch.tensor(n_new, device=cuda), cache, return_all=True)
        assert cache.kv_len.tolist() == [P + E + n for n in n_new]
        dec = []
        for i in range(N):
            step = torch.stack([tok[b, P + E + n_new[b] + i] for b in range(B)])
            dec.append(inf.decode_step(m, step, cache))
    e_full = e_ext = 0.0
    for b in range(B):
        got = torch.cat([first[b:b + 1], ext[b], rag[b, :n_new[b]], torch.stack([d[b] for d in dec])]).float()
        assert got.shape == ref[b].shape
        e_full = max(e_full, (full[b] - ref[b]).abs().max().item())
        e_ext = max(e_ext, (got - ref[b]).abs().max().item())
    print(f"e_full = {e_full:.3e}, e_ext = {e_ext:.3e}")
    assert e_ext <= 2 * e_full + 1e-3


@pytest.mark.parametrize("preset,over", CONFIGS)
def test_chunked_prefill_logits_vs_fp32_model(cuda, preset, over):
    """bf16, a 40-column prompt with lens [40, 23] in pieces of 16: the logits of rows lens - 1 under the rule of
    test_extend_logits_vs_fp32_model, kv_len equal to the one-shot prefill's and every cache row within the
    bf16 output bound of it.

    Measured on MI355X: llama-tiny e_full 7.824e-3, e_chunk 7.824e-3, cache rows bit-equal; head_dim-128 GQA 4:1
    e_full 8.564e-3, e_chunk 8.564e-3, max |k - k_one| 1.172e-2, max |v - v_one| 7.812e-3 (one bf16 ulp)."""
    cfg, m32, m = _models(cuda, preset, over)
    B, S = 2, 40
    lens = [40, 23]
    tok = torch.randint(0, cfg.vocab_size, (B, S), device=cuda)
    lt = torch.tensor(lens, device=cuda)
    bi = torch.arange(B, device=cuda)
    with torch.no_grad():
        ref = _ref_forward(m32, tok)[bi, lt - 1]
        full = m(tok).float()[bi, lt - 1]
        one = inf.KVCache(cfg, B, 64, torch.bfloat16, cuda)
        inf.prefill(m, tok, lt, one)
        cache = inf.KVCache(cfg, B, 64, torch.bfloat16, cuda)
        got = inf.prefill(m, tok, lt, cache, chunk=16).float()
    e_full, e_chunk = (full - ref).abs().max().item(), (got - ref).abs().max().item()
    ek = max((a[:, :S].float() - b[:, :S].float()).abs().max().item() for a, b in zip(cache.k, one.k))
    ev = max((a[:, :S].float() - b[:, :S].float()).abs().max().item() for a, b in zip(cache.v, one.v))
    print(f"e_full = {e_full:.3e}, e_chunk = {e_chunk:.3e}, |k - k_one| = {ek:.3e}, |v - v_one| = {ev:.3e}")
    assert cache.kv_len.tolist() == lens == one.kv_len.tolist()
    assert e_chunk <= 2 * e_full + 1e-3
    assert ek < O_TOL and ev < O_TOL


def test_fp32_extend_on_torch_math_matches_cpu(cuda):
    """An fp32 model on the GPU extends through attention_extend_ref / rope_append_ref."""
    torch.manual_seed(0)
    cfg = get_preset("llama-micro", seq_len=48)
    mc = Transformer(cfg).float().eval()
    mg = Transformer(cfg).float().to(cuda).eval()
    mg.load_state_dict(mc.state_dict())
    tok = torch.randint(0, cfg.vocab_size, (2, 24))
    outs = []
    for m, dev in ((mc, "cpu"), (mg, cuda)):
        cache = inf.KVCache(cfg, 2, 24, torch.float32, dev)
        t = tok.to(dev)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)  # the once-per-shape note of the torch-math path
            rows = [inf.prefill(m, t[:, :8], torch.tensor([8, 5]), cache)]
            rows.append(inf.extend(m, t[:, 8:14], torch.tensor([6, 2]), cache))
            rows.append(inf.extend(m, t[:, 14:15], torch.tensor([1, 1]), cache))
            rows.append(inf.prefill(m, t[:, :11], torch.tensor([11, 7]), inf.KVCache(cfg, 2, 24, torch.float32, dev),
                                    chunk=4))
        assert cache.kv_len.tolist() == [15, 8]
        outs.append(torch.stack(rows, 1).cpu())
    assert (outs[0] - outs[1]).abs().max().item() < 1e-4
