"""extend on an fp8 KV cache (csrc/kernels/attention_extend_fp8.hip, the T-token rope_append_fp8): bits of the
quantizing append, both arms of attn_extend_fp8 against the fp64 oracle on the dequantized cache and their bit
contract, and extend / chunked prefill with fp8_extend=True against the fp32 model on its own fp8 cache."""
import copy
import functools
import math
import warnings

import pytest
import torch

from pyrecover_amd import _ext
from pyrecover_amd import inference as inf
from pyrecover_amd.ops import reference as R
from tests import kv_fp8_oracles as Q
from tests.test_extend_gpu import CONFIGS, LSE_TOL, O_TOL, _inputs, _lens, _models, _rope_case
from tests.test_extend_split_gpu import _xc_bases
from tests.test_kv_fp8_gpu import _fp8_caches

pytestmark = pytest.mark.gpu
SPLIT = pytest.mark.parametrize("split", [0, 1])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Hq,Hkv", [(4, 4), (8, 1)])
def test_rope_append_fp8_multi_token_bits(cuda, Hq, Hkv, D, dtype):
    """B * T = 15 rows: the last wave is partial wherever it can be (at Hq + 2 Hkv = 12, D = 128 a row is 192 lanes,
    three whole waves, for any row count). q bit-equal to rope_append_, every stored row and scale the oracle's
    quantization of the row the 16-bit op wrote, the rest untouched; bases cap - 2 and cap + 9 overflow."""
    C = _ext.native()
    cap, B, T = 40, 3, 5
    tab, qkv, _, _ = _rope_case(cuda, B, T, cap, Hq, Hkv, D, dtype)
    for base in ([0, 7, cap - 2], [-2, cap + 9, cap - T]):
        n, q16, q8 = _lens(cuda, base), qkv.clone(), qkv.clone()
        kc, vc = (torch.zeros(B, cap, Hkv, D, dtype=dtype, device=cuda) for _ in range(2))
        C.rope_append_(q16, tab, n, kc, vc)
        got = _fp8_caches(cuda, B, cap, Hkv, D)
        C.rope_append_fp8_(q8, tab, n, *got)
        assert torch.equal(q8, q16)
        want = [t.cpu() for t in _fp8_caches(cuda, B, cap, Hkv, D)]
        for b in range(B):
            rows = slice(min(max(base[b], 0), cap), min(max(base[b], 0) + T, cap))
            if rows.start < cap:
                want[0][b, rows], want[2][b, rows] = Q.quantize(kc[b, rows].cpu())
                want[1][b, rows], want[3][b, rows] = Q.quantize(vc[b, rows].cpu())
        assert all(torch.equal(g.cpu(), w) for g, w in zip(got, want))


def _quantized(x):  # x's cache bytes and scales by the rule and their fp64 dequantization (computed on the CPU)
    q, s = R.kv_quantize_ref(x.cpu())
    return q.to(x.device), s.to(x.device), R.kv_dequantize_ref(q, s, torch.float64).to(x.device)


@functools.lru_cache(maxsize=1)
def _case(cuda, dtype, D, T, Hq, Hkv, seed=0):
    """test_attn_extend_split_vs_reference's inputs, every (token, head) row of K and of V times its own power of two in
    2^-6 .. 2^6, quantized; the fp64 oracle on the dequantized caches; mag: the oracle's output for V rows that hold their
    multiplier, the V magnitude a row mixes, which O_TOL (absolute, unit-scale V) is relative to."""
    XC, base = _xc_bases()
    q, k, v = _inputs(cuda, len(base), T, 2 * XC + 150, Hq, Hkv, D, dtype, seed)
    mk, mv = (torch.ldexp(torch.ones_like(k[..., :1], dtype=torch.float32),
                          torch.randint(-6, 7, k[..., :1].shape, device=cuda)) for _ in range(2))
    (kq, ks, kd), (vq, vs, vd) = _quantized((k.float() * mk).to(dtype)), _quantized((v.float() * mv).to(dtype))
    n, scale = _lens(cuda, base), 1 / math.sqrt(D)
    o_ref, lse_ref = R.attention_extend_ref(q.double(), kd, vd, n, scale)
    mag = R.attention_extend_ref(q.double(), kd, mv.double().expand_as(vd), n, scale)[0][..., :1]
    return q, (kq, vq, ks, vs), n, o_ref, lse_ref, mag


@SPLIT
@pytest.mark.parametrize("T,Hq,Hkv", [(5, 2, 2), (33, 8, 1), (135, 2, 2), (8, 4, 1)])
@pytest.mark.parametrize("dtype,D", [(torch.bfloat16, 128), (torch.float16, 128), (torch.bfloat16, 64)])
def test_attn_extend_fp8_vs_reference(cuda, dtype, D, T, Hq, Hkv, split):
    """4, 2 and 1 waves per sub-tile, ragged row tiles and an exactly full wave over three chunks, single pass and
    key split. The dequantized operands are exact in 16 bits: the 16-bit kernel's rounding points and bounds."""
    q, caches, n, o_ref, lse_ref, mag = _case(cuda, dtype, D, T, Hq, Hkv)
    o, lse = _ext.native().attn_extend_fp8(q, *caches, n, 1 / math.sqrt(D), split=split)
    assert o.dtype == q.dtype and lse.dtype == torch.float32 and o.shape == q.shape and lse.shape == q.shape[:3]
    eo, el = ((o.double() - o_ref).abs() / mag).max().item(), (lse - lse_ref).abs().max().item()
    print(f"|o - o_ref| / mag = {eo:.3e}, |lse - lse_ref| = {el:.3e}")
    assert eo < O_TOL and el < LSE_TOL  # a non-finite o or lse fails here too


@SPLIT
def test_attn_extend_fp8_bits(cuda, split):
    """Equal bits for a fixed split: run to run, each sequence alone against the ragged batch, the same contents
    in a longer cache, and a poisoned tail beyond kv_len + T (NaN bytes, NaN / Inf scales) against a zero tail."""
    C = _ext.native()
    XC, base = _xc_bases()
    T, scale = 33, 1 / math.sqrt(128)
    q, c8, n, _, _, _ = _case(cuda, torch.bfloat16, 128, T, 8, 1, seed=1)
    o, lse = C.attn_extend_fp8(q, *c8, n, scale, split=split)

    def same(c_, s=slice(None)):
        o2, lse2 = C.attn_extend_fp8(q[s], *(t[s] for t in c_), n[s], scale, split=split)
        return torch.equal(o2, o[s]) and torch.equal(lse2, lse[s])

    assert same(c8) and all(same(c8, slice(b, b + 1)) for b in range(len(base)))
    assert same([torch.cat([t, torch.full_like(t[:, :XC + 64], 3)], 1) for t in c8])
    zero, poison = [t.clone() for t in c8], [t.clone() for t in c8]
    for b, L in enumerate(base):
        for t in zero:
            t[b, L + T:] = 0
        poison[0][b, L + T:], poison[1][b, L + T:] = 0x7F, 0xFF
        poison[2][b, L + T:], poison[3][b, L + T:L + T + 3], poison[3][b, L + T + 3:] = math.nan, math.inf, -math.inf
    assert same(zero) and same(poison)


@SPLIT
@pytest.mark.parametrize("D,Hq,Hkv", [(128, 2, 2), (64, 8, 1)])
def test_attn_extend_fp8_late_spike(cuda, D, Hq, Hkv, split):
    """test_attn_extend_split_combine_weights's spike at the last visible key of the last row, whose K row carries
    the largest scale (2^2; no other row's is above 2^0): head 0 of that row is that key's dequantized V row."""
    XC = _xc_bases()[0]
    T, base, cap, dt = 135, XC + 20, 2 * XC + 150, torch.bfloat16
    (q, k, v), at = _inputs(cuda, 1, T, cap, Hq, Hkv, D, dt, seed=3), base + T - 1
    mk = torch.ldexp(torch.ones(1, cap, Hkv, 1, device=cuda), torch.randint(-6, 7, (1, cap, Hkv, 1), device=cuda))
    k = (k.float() * mk).to(dt)
    q[0, T - 1, 0], k[0, at, 0], v[0, at, 0] = 4.0, 1024.0, v[0, at, 0] * 32
    (kq, ks, _), (vq, vs, vd) = _quantized(k), _quantized(v)
    assert ks[0, at, 0] == 4 and ks.max() == 4
    o, _ = _ext.native().attn_extend_fp8(q, kq, vq, ks, vs, _lens(cuda, [base]), 1 / math.sqrt(D), split=split)
    assert ((o[0, T - 1, 0].double() - vd[0, at, 0]).abs() / 32).max().item() < O_TOL


def _route(m, tok, n_new, dtype, dev):
    """Prefill 40, extend 16, a ragged extend n_new and 4 decode steps on an fp8 cache, every row's logits."""
    B, P, E, N = tok.shape[0], 40, 16, 4
    cache = inf.KVCache(m.model_args, B, tok.shape[1], dtype, dev, kv_dtype="fp8")
    tok = tok.to(dev)
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # the once-per-shape note of the torch-math path
        first = inf.prefill(m, tok[:, :P], torch.full((B,), P, device=dev), cache)
        ext = inf.extend(m, tok[:, P:P + E], torch.full((B,), E, device=dev), cache, return_all=True, fp8_extend=True)
        pad = torch.arange(max(n_new), device=dev).view(1, -1) >= torch.tensor(n_new, device=dev).view(-1, 1)
        rag_tok = tok[:, P + E:P + E + max(n_new)].masked_fill(pad, 0)
        rag = inf.extend(m, rag_tok, torch.tensor(n_new, device=dev), cache, return_all=True, fp8_extend=True)
        dec = [inf.decode_step(m, torch.stack([tok[b, P + E + n_new[b] + i] for b in range(B)]), cache) for i in range(N)]
    assert cache.kv_len.tolist() == [P + E + n + N for n in n_new]
    return torch.cat([torch.cat([first[b:b + 1], ext[b], rag[b, :n_new[b]], torch.stack([d[b] for d in dec])])
                      for b in range(B)]).float().cpu()


@pytest.mark.parametrize("preset,over", CONFIGS)
def test_extend_fp8_model_vs_fp32_model(cuda, preset, over):
    """test_extend_logits_vs_fp32_model's route, then prefill(chunk=16) of 40 columns with lens [40, 23], fp8_extend=True,
    judged as test_decode_logits_fp8_cache_vs_fp32_model: fp32 and bf16 torch math on the CPU and bf16 HIP, each on its
    own fp8 cache, e_gpu <= 2 * e_ref + 1e-3; the chunked prefill's cache bytes are those of three extend calls. Measured
    on MI355X, e_ref / e_gpu: route 1.054e-2 / 9.902e-3, 1.186e-2 / 1.070e-2; chunked 8.141e-3 / 8.563e-3, 9.013e-3 / 8.741e-3."""
    cfg, g32, mg = _models(cuda, preset, over)  # the same bf16-representable weights in fp32 and bf16
    models = [(copy.deepcopy(g32).cpu(), torch.float32, "cpu"), (copy.deepcopy(mg).cpu(), torch.bfloat16, "cpu"),
              (mg, torch.bfloat16, cuda)]
    n_new, lens = [8, 3], torch.tensor([40, 23])
    tok = torch.randint(0, cfg.vocab_size, (2, 40 + 16 + max(n_new) + 4))
    caches = [inf.KVCache(cfg, 2, 64, dt, dev, kv_dtype="fp8") for _, dt, dev in models]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        chunked = [inf.prefill(m, tok[:, :40].to(dev), lens.to(dev), c, chunk=16, fp8_extend=True).float().cpu()
                   for (m, _, dev), c in zip(models, caches)]
    for name, (ref, cpu, gpu) in (("route", [_route(m, tok, n_new, dt, dev) for m, dt, dev in models]), ("chunked", chunked)):
        e_ref, e_gpu = (cpu - ref).abs().max().item(), (gpu - ref).abs().max().item()
        print(f"{name}: e_ref = {e_ref:.3e}, e_gpu = {e_gpu:.3e}")
        assert e_gpu <= 2 * e_ref + 1e-3
    steps = inf.KVCache(cfg, 2, 64, torch.bfloat16, cuda, kv_dtype="fp8")
    for c0 in (0, 16, 32):
        piece = tok[:, c0:min(c0 + 16, 40)].to(cuda)
        inf.extend(models[2][0], piece, torch.full((2,), piece.shape[1], device=cuda), steps, fp8_extend=True)
    got = caches[2]
    for a, b in zip(got.k + got.v + got.k_scale + got.v_scale, steps.k + steps.v + steps.k_scale + steps.v_scale):
        assert torch.equal(a[:, :40], b[:, :40])
