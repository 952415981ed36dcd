"""extend on an MXFP4 KV cache (csrc/kernels/attention_extend_fp4.hip): both arms of attn_extend_fp4 against the fp64
oracle on the dequantized cache and, bit for bit, against attn_extend on the cache dequantized to the query dtype; the
own-data-only contract; the bindings' checks; extend / chunked prefill with fp4_extend=True judged against fp8_extend."""
import copy
import functools
import math
import warnings

import pytest
import torch

from pyrecover_amd import _ext
from pyrecover_amd import inference as inf
from pyrecover_amd.ops import reference as R
from tests.test_extend_gpu import CONFIGS, LSE_TOL, O_TOL, _inputs, _lens, _models
from tests.test_extend_split_gpu import _xc_bases

pytestmark = pytest.mark.gpu
SPLIT = pytest.mark.parametrize("split", [0, 1])


def _quantized(x):  # x's nibbles and scale bytes by the rule, dequantized to fp64 and (exactly) to x's dtype
    q, s = R.kv_quantize_fp4_ref(x.cpu())
    return [t.to(x.device) for t in (q, s, R.kv_dequantize_fp4_ref(q, s, torch.float64), R.kv_dequantize_fp4_ref(q, s, x.dtype))]


@functools.lru_cache(maxsize=1)
def _case(cuda, dtype, D, T, Hq, Hkv, seed=0):
    """test_extend_fp8_gpu._case with the fp4 rule: every (token, head) row of K and of V times its own power of two
    in 2^-6 .. 2^6, so that block scales differ within a tile; the fp64 oracle on the dequantized caches and mag."""
    XC, base = _xc_bases()
    q, k, v = _inputs(cuda, len(base), T, 2 * XC + 150, Hq, Hkv, D, dtype, seed)
    mk, mv = (torch.ldexp(torch.ones_like(k[..., :1], dtype=torch.float32),
                          torch.randint(-6, 7, k[..., :1].shape, device=cuda)) for _ in range(2))
    (kq, ks, kd, k16), (vq, vs, vd, v16) = _quantized((k.float() * mk).to(dtype)), _quantized((v.float() * mv).to(dtype))
    assert torch.equal(k16.double(), kd) and torch.equal(v16.double(), vd)
    n, scale = _lens(cuda, base), 1 / math.sqrt(D)
    o_ref, lse_ref = R.attention_extend_ref(q.double(), kd, vd, n, scale)
    mag = R.attention_extend_ref(q.double(), kd, mv.double().expand_as(vd), n, scale)[0][..., :1]
    return q, (kq, vq, ks, vs), n, o_ref, lse_ref, mag, (k16, v16)


@SPLIT
@pytest.mark.parametrize("T,Hq,Hkv", [(5, 2, 2), (33, 8, 1), (135, 2, 2), (8, 4, 1)])
@pytest.mark.parametrize("dtype,D", [(torch.bfloat16, 128), (torch.float16, 128), (torch.bfloat16, 64)])
def test_attn_extend_fp4_vs_reference_and_16bit_kernel(cuda, dtype, D, T, Hq, Hkv, split):
    """4, 2 and 1 waves per sub-tile, ragged row tiles and an exactly full wave over three chunks. The dequantized operands are
    exact in 16 bits: the 16-bit kernel's bounds and, for a fixed split, its bits (a wrong lane map, nibble order or scale changes them)."""
    C = _ext.native()
    q, caches, n, o_ref, lse_ref, mag, (k16, v16) = _case(cuda, dtype, D, T, Hq, Hkv)
    o, lse = C.attn_extend_fp4(q, *caches, n, 1 / math.sqrt(D), split=split)
    assert o.dtype == q.dtype and lse.dtype == torch.float32 and o.shape == q.shape and lse.shape == q.shape[:3]
    eo, el = ((o.double() - o_ref).abs() / mag).max().item(), (lse - lse_ref).abs().max().item()
    print(f"|o - o_ref| / mag = {eo:.3e}, |lse - lse_ref| = {el:.3e}")
    assert eo < O_TOL and el < LSE_TOL  # a non-finite o or lse fails here too
    o16, lse16 = C.attn_extend(q, k16, v16, n, 1 / math.sqrt(D), split)
    assert torch.equal(o, o16) and torch.equal(lse, lse16)


@SPLIT
def test_attn_extend_fp4_bits(cuda, split):
    """Equal bits for a fixed split: run to run, each sequence alone against the ragged batch, the same contents in a longer
    cache, and a poisoned tail beyond kv_len + T (0xFF nibble bytes, scale bytes 0xFF then 0x00) against a zero tail."""
    C = _ext.native()
    XC, base = _xc_bases()
    T, scale = 33, 1 / math.sqrt(128)
    q, c4, n = _case(cuda, torch.bfloat16, 128, T, 8, 1, seed=1)[:3]
    o, lse = C.attn_extend_fp4(q, *c4, n, scale, split=split)

    def same(c_, s=slice(None)):
        o2, lse2 = C.attn_extend_fp4(q[s], *(t[s].contiguous() for t in c_), n[s], scale, split=split)
        return torch.equal(o2, o[s]) and torch.equal(lse2, lse[s])

    assert same(c4) and all(same(c4, slice(b, b + 1)) for b in range(len(base)))
    assert same([torch.cat([t, torch.full_like(t[:, :XC + 64], 3)], 1) for t in c4])
    zero, poison = [t.clone() for t in c4], [t.clone() for t in c4]
    for b, L in enumerate(base):
        for t in zero:
            t[b, L + T:] = 0
        poison[0][b, L + T:], poison[1][b, L + T:] = 0xFF, 0xFF
        poison[2][b, L + T:], poison[3][b, L + T:L + T + 3], poison[3][b, L + T + 3:] = 0xFF, 0xFF, 0x00
    assert same(zero) and same(poison)


def test_attn_extend_fp4_binding_rejects_bad_arguments(cuda):
    C = _ext.native()
    D, Hq, Hkv, cap, T = 64, 4, 2, 32, 3
    q = _inputs(cuda, 2, T, cap, Hq, Hkv, D, torch.bfloat16)[0]
    kq = torch.zeros(2, cap, Hkv, D // 2, dtype=torch.uint8, device=cuda)
    ks, n = torch.full((2, cap, Hkv, D // 32), 127, dtype=torch.uint8, device=cuda), _lens(cuda, [3, 4])
    C.attn_extend_fp4(q, kq, kq, ks, ks, n, 0.125)  # the good call
    k2, s2 = kq.repeat(1, 1, 1, 2), ks.repeat(1, 1, 1, 2)  # a head_dim 128 cache under head_dim 64 queries
    bad = [("k_scale and v_scale", lambda: C.attn_extend_fp4(q, kq, kq, ks.float(), ks.float(), n, 0.125)),
           ("k_scale and v_scale", lambda: C.attn_extend_fp4(q, kq, kq, ks[..., :1].contiguous(), ks, n, 0.125)),
           ("disagree on head_dim", lambda: C.attn_extend_fp4(q, k2, k2, s2, s2, n, 0.125)),
           ("split must be", lambda: C.attn_extend_fp4(q, kq, kq, ks, ks, n, 0.125, split=2)),
           ("split must be", lambda: C.attn_extend_fp4(q, kq, kq, ks, ks, n, 0.125, split=-2))]
    for match, call in bad:
        with pytest.raises(RuntimeError, match=match):
            call()


def _route(m, tok, n_new, dtype, dev, kind):
    """Prefill 40, extend 16, a ragged extend n_new and 4 decode steps on a cache of ``kind``, every row's logits."""
    B, P, E, N = tok.shape[0], 40, 16, 4
    cache, opt = inf.KVCache(m.model_args, B, tok.shape[1], dtype, dev, kv_dtype=kind), dict(fp8_extend=True, fp4_extend=True)
    tok = tok.to(dev)
    first = inf.prefill(m, tok[:, :P], torch.full((B,), P, device=dev), cache)
    ext = inf.extend(m, tok[:, P:P + E], torch.full((B,), E, device=dev), cache, return_all=True, **opt)
    pad = torch.arange(max(n_new), device=dev).view(1, -1) >= torch.tensor(n_new, device=dev).view(-1, 1)
    rag_tok = tok[:, P + E:P + E + max(n_new)].masked_fill(pad, 0)
    rag = inf.extend(m, rag_tok, torch.tensor(n_new, device=dev), cache, return_all=True, **opt)
    dec = [inf.decode_step(m, torch.stack([tok[b, P + E + n_new[b] + i] for b in range(B)]), cache) for i in range(N)]
    assert cache.kv_len.tolist() == [P + E + n + N for n in n_new]
    return torch.cat([torch.cat([first[b:b + 1], ext[b], rag[b, :n_new[b]], torch.stack([d[b] for d in dec])])
                      for b in range(B)]).float().cpu()


@pytest.mark.parametrize("preset,over", CONFIGS)
def test_extend_fp4_model_vs_fp32_model(cuda, preset, over):
    """test_extend_fp8_model_vs_fp32_model's route, then prefill(chunk=16) of 40 columns with lens [40, 23], on fp8 and on
    fp4 caches in the same run: e = max |bf16 HIP logits - fp32 torch-math logits on the CPU|, each model on its own
    cache of that kind, and e_fp4 <= 2 * e_fp8 as test_decode_logits_fp4_cache_vs_fp64_reference judges the decode step.
    Measured on MI355X, e_fp8 / e_fp4: route 9.902e-3 / 1.236e-2, 1.070e-2 / 1.229e-2; chunked 8.563e-3 / 1.122e-2,
    8.741e-3 / 1.125e-2 (profiles/decode/README.md)."""
    cfg, g32, mg = _models(cuda, preset, over)  # the same bf16-representable weights in fp32 and bf16
    models = [(copy.deepcopy(g32).cpu(), torch.float32, "cpu"), (mg, torch.bfloat16, cuda)]
    n_new, lens = [8, 3], torch.tensor([40, 23])
    tok = torch.randint(0, cfg.vocab_size, (2, 40 + 16 + max(n_new) + 4))
    e = {}
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # the once-per-shape note of the torch-math path
        for kind in ("fp8", "fp4"):
            ref, gpu = (_route(m, tok, n_new, dt, dev, kind) for m, dt, dev in models)
            caches = [inf.KVCache(cfg, 2, 64, dt, dev, kv_dtype=kind) for _, dt, dev in models]
            cref, cgpu = (inf.prefill(m, tok[:, :40].to(dev), lens.to(dev), c, chunk=16, fp8_extend=True,
                                      fp4_extend=True).float().cpu() for (m, _, dev), c in zip(models, caches))
            e[kind] = ((gpu - ref).abs().max().item(), (cgpu - cref).abs().max().item())
    print(f"route: e_fp8 = {e['fp8'][0]:.3e}, e_fp4 = {e['fp4'][0]:.3e}; chunked: e_fp8 = {e['fp8'][1]:.3e}, e_fp4 = {e['fp4'][1]:.3e}")
    assert e["fp4"][0] <= 2 * e["fp8"][0] and e["fp4"][1] <= 2 * e["fp8"][1]
