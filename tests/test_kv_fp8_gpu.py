"""fp8 KV cache on the GPU (csrc/kernels/attention_decode_fp8.hip): the quantizing stores bit for bit against
the oracle of tests/kv_fp8_oracles.py applied to what the 16-bit path holds, attn_decode_fp8 against the fp64
oracle on the dequantized cache (row-scaled error, as tests/test_attention_rowerr_gpu.py judges attn_decode),
its bit contracts, the bindings' argument checks, and the model level: logits against the fp32 model, the
captured decode step, and generate.py --kv-cache-dtype fp8 from a train.py checkpoint."""
import json
import os
import subprocess
import sys
import warnings

import pytest
import torch

from pyrecover_amd import _ext
from pyrecover_amd import inference as inf
from pyrecover_amd.config import get_preset
from pyrecover_amd.models.llama import Transformer
from pyrecover_amd.ops import reference as R
from tests import attention_oracles as A
from tests import kv_fp8_oracles as Q
from tests.test_attention_rowerr_gpu import Judge

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = (torch.bfloat16, torch.float16)
HEADS = [(4, 4), (4, 2), (8, 2), (8, 1)]
BYTE, SCALE = 0xAB, 7.0  # what an untouched cache row and scale hold in the store tests


def _lens(cuda, lens):
    return torch.tensor(lens, device=cuda, dtype=torch.int32)


def _fp8_caches(cuda, B, cap, Hkv, D):
    kq = torch.full((B, cap, Hkv, D), BYTE, dtype=torch.uint8, device=cuda)
    ks = torch.full((B, cap, Hkv), SCALE, dtype=torch.float32, device=cuda)
    return kq, kq.clone(), ks, ks.clone()


def _strided(x, pad=24):
    """The same values as rows of a wider buffer: row stride > the row's width."""
    base = torch.zeros(x.shape[0], x.shape[1] + pad, dtype=x.dtype, device=x.device)
    base[:, :x.shape[1]] = x
    return base[:, :x.shape[1]]


def _eq(got, want):
    return torch.equal(got.cpu(), want)


@pytest.mark.parametrize("dtype", DTYPES, ids=A.dname)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_kv_quantize_bits(cuda, Hq, Hkv, D, dtype):
    """The prefill store: k / v views of a strided fused QKV activation (edge rows of the rule among them)
    into cache rows 0 .. S - 1, bit-equal to the oracle; rows S .. cap - 1 and their scales untouched."""
    C = _ext.native()
    B, S, cap = 3, 7, 10
    nq, nk = Hq * D, Hkv * D
    torch.manual_seed(0)
    act = (torch.randn(B * S, nq + 2 * nk, device=cuda) * 3).to(dtype)
    edges = Q.edge_rows(dtype, D).to(cuda)
    n = min(len(edges), B * S * Hkv)
    kpart =act[:, nq:nq + nk].reshape(B * S * Hkv, D).clone()
    kpart[:n] = edges[:n]
    act[:, nq:nq + nk] = kpart.view(B * S, nk)
    vpart = act[:, nq + nk:].reshape(B * S * Hkv, D).clone()
    vpart[-n:] = edges[:n]
    act[:, nq + nk:] = vpart.view(B * S, nk)
    qkv = _strided(act)
    assert qkv.stride(0) > nq + 2 * nk
    k = qkv[:, nq:nq + nk].view(B, S, Hkv, D)
    v = qkv[:, nq + nk:].view(B, S, Hkv, D)
    kq, vq, ks, vs = _fp8_caches(cuda, B, cap, Hkv, D)
    C.kv_quantize_(k, v, kq, vq, ks, vs)
    for x, q, s in ((k, kq, ks), (v, vq, vs)):
        wq, ws = Q.quantize(x.cpu())
        assert _eq(q[:, :S], wq) and _eq(s[:, :S], ws)
        assert bool((q[:, S:] == BYTE).all()) and bool((s[:, S:] == SCALE).all())
    assert torch.equal(qkv, act)  # the activation is read only


@pytest.mark.parametrize("dtype", DTYPES, ids=A.dname)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_rope_append_fp8_bits(cuda, Hq, Hkv, D, dtype):
    """q bit-equal to rope_append_; the cache row is the oracle applied to the row rope_append_ writes into a
    16-bit cache; every other row and scale untouched; kv_len 0, 5, cap - 1, and lengths outside the cache."""
    C = _ext.native()
    B, cap = 3, 40
    nq, nk = Hq * D, Hkv * D
    tab = R.rope_table(R.precompute_freqs_cis(D, cap)).to(cuda)
    torch.manual_seed(1)
    act = (torch.randn(B, nq + 2 * nk, device=cuda) * 2).to(dtype)
    for lens in ([0, 5, cap - 1], [-2, cap + 9, 5]):
        pos = [min(max(n, 0), cap - 1) for n in lens]
        n = _lens(cuda, lens)
        q16 = act.clone()
        kc16, vc16 = torch.zeros(B, cap, Hkv, D, dtype=dtype, device=cuda), torch.zeros(B, cap, Hkv, D, dtype=dtype, device=cuda)
        C.rope_append_(q16, tab, n, kc16, vc16)
        q8 = _strided(act)
        kq, vq, ks, vs = _fp8_caches(cuda, B, cap, Hkv, D)
        C.rope_append_fp8_(q8, tab, n, kq, vq, ks, vs)
        assert torch.equal(q8, q16)  # q rotated, the k / v columns of the activation as they were
        want = [t.cpu() for t in _fp8_caches(cuda, B, cap, Hkv, D)]
        for b, p in enumerate(pos):
            want[0][b, p], want[2][b, p] = Q.quantize(kc16[b, p].cpu())
            want[1][b, p], want[3][b, p] = Q.quantize(vc16[b, p].cpu())
        for got, w in zip((kq, vq, ks, vs), want):
            assert _eq(got, w)


@pytest.mark.parametrize("dtype", DTYPES, ids=A.dname)
@pytest.mark.parametrize("D", [64, 128])
def test_rope_append_fp8_edge_rows(cuda, D, dtype):
    """Position 0 rotates by the identity, so the rule's edge rows reach the quantizing store as they are, as k
    and as v rows; more than one grid stride of work."""
    C = _ext.native()
    Hq, Hkv, cap = 2, 2, 4
    edges = Q.edge_rows(dtype, D)
    B = (len(edges) + Hkv - 1) // Hkv
    rows = torch.zeros(B * Hkv, D, dtype=dtype)
    rows[:len(edges)] = edges
    nq, nk = Hq * D, Hkv * D
    act = torch.randn(B, nq + 2 * nk).to(dtype)
    act[:, nq:nq + nk] = rows.view(B, nk)
    act[:, nq + nk:] = rows.flip(0).view(B, nk)
    tab = R.rope_table(R.precompute_freqs_cis(D, cap)).to(cuda)
    q8 = _strided(act.to(cuda))
    kq, vq, ks, vs = _fp8_caches(cuda, B, cap, Hkv, D)
    C.rope_append_fp8_(q8, tab, _lens(cuda, [0] * B), kq, vq, ks, vs)
    wq, ws = Q.quantize(rows.view(B, Hkv, D))
    assert _eq(kq[:, 0], wq) and _eq(ks[:, 0], ws)
    wq, ws = Q.quantize(rows.flip(0).view(B, Hkv, D))
    assert _eq(vq[:, 0], wq) and _eq(vs[:, 0], ws)
    assert bool((kq[:, 1:] == BYTE).all()) and bool((vs[:, 1:] == SCALE).all())


def test_rope_append_fp8_grid_stride(cuda):
    """More work items than one pass of the launch grid (2048 blocks of 256), with a ragged tail."""
    C = _ext.native()
    Hq, Hkv, D, cap, B = 4, 4, 128, 3, 2731  # 2731 * 12 * 16 = 524352 items > 2048 * 256 = 524288
    dtype = torch.bfloat16
    nq, nk = Hq * D, Hkv * D
    tab = R.rope_table(R.precompute_freqs_cis(D, cap)).to(cuda)
    torch.manual_seed(2)
    act = torch.randn(B, nq + 2 * nk, device=cuda).to(dtype)
    n = (torch.arange(B, device=cuda) % cap).int()
    q16 = act.clone()
    kc16, vc16 = torch.zeros(B, cap, Hkv, D, dtype=dtype, device=cuda), torch.zeros(B, cap, Hkv, D, dtype=dtype, device=cuda)
    C.rope_append_(q16, tab, n, kc16, vc16)
    q8 = act.clone()
    kq, vq, ks, vs = _fp8_caches(cuda, B, cap, Hkv, D)
    C.rope_append_fp8_(q8, tab, n, kq, vq, ks, vs)
    assert torch.equal(q8, q16)
    bi = torch.arange(B, device=cuda)
    wq, ws = Q.quantize(kc16[bi, n.long()].cpu())
    assert _eq(kq[bi, n.long()], wq) and _eq(ks[bi, n.long()], ws)
    wq, ws = Q.quantize(vc16[bi, n.long()].cpu())
    assert _eq(vq[bi, n.long()], wq) and _eq(vs[bi, n.long()], ws)


# ---------------------------------------------------------------------------------------
def _case_dev(c, cuda):
    return [t.to(cuda) for t in (c.q[:, 0], c.kq, c.vq, c.ks, c.vs, c.kv_len)]


@pytest.mark.parametrize("dtype", DTYPES, ids=A.dname)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Hq,Hkv", Q.GROUPS)
def test_attn_decode_fp8_row_error(cuda, Hq, Hkv, D, dtype):
    """rho <= cap(dtype, "decode_o") = 2 u against the fp64 oracle on the dequantized cache, lse within
    lse_bound. The cap is derived: the dequantized K and V are exact in 16 bits, the scales are powers of two,
    P and the partials stay fp32, so the only 16-bit rounding on the way to o is its store (n_round = 1), as
    in the 16-bit kernel. tests/test_kv_fp8.py holds the torch reference to the same cap on the same cases."""
    C = _ext.native()
    KC = C.attn_decode_fp8_chunk()
    J = Judge("decode_fp8")
    for name in Q.RECIPES:
        c = Q.decode_case(name, D, dtype, Hq, Hkv, KC)
        assert c.kv_len.tolist() == [1, KC - 1, KC, KC + 1, 3 * KC + 17]
        q, kq, vq, ks, vs, n = _case_dev(c, cuda)
        o, lse = C.attn_decode_fp8(q, kq, vq, ks, vs, n, c.scale)
        o2, lse2 = C.attn_decode_fp8(q, kq, vq, ks, vs, n, c.scale)
        assert o.dtype == dtype and lse.dtype == torch.float32
        J.same(c, "decode_fp8", (o, lse), (o2, lse2))
        J.row(c, "decode_fp8", "o", o[:, None], c.o, c.m_o, A.cap(dtype, "decode_o"))
        J.lse(c, "decode_fp8", lse[:, :, None])
    J.done()


def test_attn_decode_fp8_bits(cuda):
    """A sequence's output is a function of its own q, bytes, scales and length alone: alone or in a ragged
    batch, at another cap, and whatever the cache holds at and beyond kv_len (NaN bytes 0x7F, NaN scales);
    length 0 gives o = 0 and lse = -inf."""
    C = _ext.native()
    KC = C.attn_decode_fp8_chunk()
    c = Q.decode_case("peaked", 128, torch.bfloat16, 8, 1, KC)
    q, kq, vq, ks, vs, _ = _case_dev(c, cuda)
    L = 2 * KC + 3
    n = _lens(cuda, [KC + 1, L, 1, 0, KC])
    o, lse = C.attn_decode_fp8(q, kq, vq, ks, vs, n, c.scale)
    assert torch.equal(o[3], torch.zeros_like(o[3])) and bool(torch.isneginf(lse[3]).all())
    assert bool(torch.isfinite(o).all()) and bool(torch.isfinite(lse[[0, 1, 2, 4]]).all())
    one = [t[1:2].contiguous() for t in (q, kq, vq, ks, vs)]
    oa, la = C.attn_decode_fp8(*one, _lens(cuda, [L]), c.scale)
    assert torch.equal(oa[0], o[1]) and torch.equal(la[0], lse[1])
    # ... in a larger cache whose tail is poisoned, against a zero tail
    big = 4 * KC + 64
    Hkv, D = 1, 128
    tails = []
    for poison in (True, False):
        kb = torch.zeros(1, big, Hkv, D, dtype=torch.uint8, device=cuda)
        vb, sk, sv = kb.clone(), torch.ones(1, big, Hkv, device=cuda), torch.ones(1, big, Hkv, device=cuda)
        kb[0, :L], vb[0, :L], sk[0, :L], sv[0, :L] = kq[1, :L], vq[1, :L], ks[1, :L], vs[1, :L]
        if poison:
            kb[0, L:], vb[0, L:] = 0x7F, 0xFF
            sk[0, L:], sv[0, L:] = float("nan"), float("inf")
            sk[0, L + 1], vb[0, L + 2] = float("-inf"), 0x7E
        tails.append(C.attn_decode_fp8(one[0], kb, vb, sk, sv, _lens(cuda, [L]), c.scale))
    for ob, lb in tails:
        assert torch.equal(ob[0], o[1]) and torch.equal(lb[0], lse[1])
    # lengths outside [0, cap] clamp
    cap = kq.shape[1]
    a = C.attn_decode_fp8(q, kq, vq, ks, vs, _lens(cuda, [-3, 0, cap + 5, 1, 2]), c.scale)
    b = C.attn_decode_fp8(q, kq, vq, ks, vs, _lens(cuda, [0, 0, cap, 1, 2]), c.scale)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_fp8_bindings_reject_bad_arguments(cuda):
    C = _ext.native()
    D, Hq, Hkv, cap, B = 64, 4, 2, 32, 2
    q = torch.randn(B, Hq, D, device=cuda).bfloat16()
    kq, vq, ks, vs = _fp8_caches(cuda, B, cap, Hkv, D)
    n = _lens(cuda, [3, 4])
    tab = R.rope_table(R.precompute_freqs_cis(D, cap)).to(cuda)
    qkv = torch.randn(B, (Hq + 2 * Hkv) * D, device=cuda).bfloat16()
    k16 = torch.randn(B, 4, Hkv, D, device=cuda).bfloat16()
    C.attn_decode_fp8(q, kq, vq, ks, vs, n, 0.125)  # the good calls
    C.rope_append_fp8_(qkv.clone(), tab, n, kq, vq, ks, vs)
    C.kv_quantize_(k16, k16.clone(), kq, vq, ks, vs)
    with pytest.raises(RuntimeError, match="bf16 or fp16"):
        C.attn_decode_fp8(q.float(), kq, vq, ks, vs, n, 0.125)
    with pytest.raises(RuntimeError, match="uint8"):
        C.attn_decode_fp8(q, kq.bfloat16(), vq.bfloat16(), ks, vs, n, 0.125)
    with pytest.raises(RuntimeError, match="uint8"):
        C.attn_decode_fp8(q, kq, vq.view(torch.int8), ks, vs, n, 0.125)
    with pytest.raises(RuntimeError, match="v_cache must have"):
        C.attn_decode_fp8(q, kq, vq[:, :-1].contiguous(), ks, vs, n, 0.125)
    with pytest.raises(RuntimeError, match="k_scale and v_scale"):
        C.attn_decode_fp8(q, kq, vq, ks[:, :-1].contiguous(), vs, n, 0.125)
    with pytest.raises(RuntimeError, match="k_scale and v_scale"):
        C.attn_decode_fp8(q, kq, vq, ks, vs.double(), n, 0.125)
    with pytest.raises(RuntimeError, match="k_scale and v_scale"):
        C.attn_decode_fp8(q, kq, vq, ks.unsqueeze(-1), vs, n, 0.125)
    with pytest.raises(RuntimeError, match="k_scale and v_scale"):
        C.attn_decode_fp8(q, kq, vq, ks.transpose(1, 2).contiguous().transpose(1, 2), vs, n, 0.125)
    with pytest.raises(RuntimeError, match="must be on"):
        C.attn_decode_fp8(q, kq.cpu(), vq, ks, vs, n, 0.125)
    with pytest.raises(RuntimeError, match="must be on"):
        C.attn_decode_fp8(q, kq, vq, ks, vs.cpu(), n, 0.125)
    with pytest.raises(RuntimeError, match="must be on"):
        C.attn_decode_fp8(q, kq, vq, ks, vs, n.cpu(), 0.125)
    with pytest.raises(RuntimeError, match="int32"):
        C.attn_decode_fp8(q, kq, vq, ks, vs, n.long(), 0.125)
    with pytest.raises(RuntimeError, match="head_dim"):
        C.attn_decode_fp8(torch.randn(B, Hq, 96, device=cuda).bfloat16(), *_fp8_caches(cuda, B, cap, Hkv, 96), n, 0.1)
    with pytest.raises(RuntimeError, match="disagree on head_dim"):
        C.attn_decode_fp8(torch.randn(B, Hq, 128, device=cuda).bfloat16(), kq, vq, ks, vs, n, 0.1)
    with pytest.raises(RuntimeError, match="multiple of n_kv_heads"):
        C.attn_decode_fp8(q[:, :3].contiguous(), kq, vq, ks, vs, n, 0.125)
    with pytest.raises(RuntimeError, match="contiguous"):
        C.attn_decode_fp8(q, kq.transpose(1, 2).contiguous().transpose(1, 2), vq, ks, vs, n, 0.125)
    mis = torch.randn(B * Hq * D + 4, device=cuda).bfloat16()[4:].view(B, Hq, D)  # 8 bytes off a 16-B boundary
    with pytest.raises(RuntimeError, match="16-B aligned"):
        C.attn_decode_fp8(mis, kq, vq, ks, vs, n, 0.125)
    with pytest.raises(RuntimeError, match="bf16 or fp16"):
        C.rope_append_fp8_(qkv.float(), tab, n, kq, vq, ks, vs)
    with pytest.raises(RuntimeError, match="k_scale and v_scale"):
        C.rope_append_fp8_(qkv.clone(), tab, n, kq, vq, ks[:1].contiguous(), vs)
    with pytest.raises(RuntimeError, match="table"):
        C.rope_append_fp8_(qkv.clone(), tab[:cap - 1].contiguous(), n, kq, vq, ks, vs)
    with pytest.raises(RuntimeError, match="qkv must be"):
        C.rope_append_fp8_(qkv[:, :-D].contiguous(), tab, n, kq, vq, ks, vs)
    with pytest.raises(RuntimeError, match="must be on"):
        C.rope_append_fp8_(qkv.clone(), tab.cpu(), n, kq, vq, ks, vs)
    with pytest.raises(RuntimeError, match="do not fit"):
        C.kv_quantize_(torch.randn(B, cap + 1, Hkv, D, device=cuda).bfloat16(),
                       torch.randn(B, cap + 1, Hkv, D, device=cuda).bfloat16(), kq, vq, ks, vs)
    with pytest.raises(RuntimeError, match="v must have"):
        C.kv_quantize_(k16, k16.half(), kq, vq, ks, vs)
    with pytest.raises(RuntimeError, match="views of rows"):
        C.kv_quantize_(k16.transpose(1, 2).contiguous().transpose(1, 2), k16.transpose(1, 2).contiguous().transpose(1, 2),
                       kq, vq, ks, vs)
    with pytest.raises(RuntimeError, match="disagree"):
        C.kv_quantize_(k16[:, :, :1].contiguous(), k16[:, :, :1].contiguous(), kq, vq, ks, vs)
    with pytest.raises(RuntimeError, match="bf16 or fp16"):
        C.kv_quantize_(k16.float(), k16.float(), kq, vq, ks, vs)


# ---------------------------------------------------------------------------------------
def _teacher_forced(m, tok, P, N, dtype, dev):
    """Logits of rows P - 1 .. P + N - 2: a P-token prefill, then N - 1 decode steps, on an fp8 cache."""
    B = tok.shape[0]
    cache = inf.KVCache(m.model_args, B, P + N, dtype, dev, kv_dtype="fp8")
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # the once-per-shape note of the torch-math path
        rows = [inf.prefill(m, tok[:, :P], torch.full((B,), P, device=dev), cache)]
        for t in range(P, P + N - 1):
            rows.append(inf.decode_step(m, tok[:, t], cache))
    assert cache.kv_len.tolist() == [P + N - 1] * B
    return torch.stack(rows, 1).float().cpu()


@pytest.mark.parametrize("preset,over", [
    ("llama-tiny", {}),  # head_dim 64, GQA 2:1
    ("llama-tiny", {"dim": 512, "n_heads": 4, "n_kv_heads": 1}),  # 2 layers, head_dim 128, GQA 4:1
])
def test_decode_logits_fp8_cache_vs_fp32_model(cuda, preset, over):
    """Teacher-forced, 64-token prefill, then 32 decode steps, every model on an fp8 cache. The yardstick is
    the fp32 model on the CPU (plain torch math, ops/reference.py with the same rule). With e_gpu the max
    abs error of the bf16 HIP logits and e_ref that of the bf16 torch-math path on the CPU (same weights,
    same tokens), require e_gpu <= 2 * e_ref + 1e-3: the same rounding points in another summation order.

    Measured on MI355X: llama-tiny e_ref 1.209e-2, e_gpu 1.288e-2; head_dim-128 GQA 4:1 e_ref 1.037e-2,
    e_gpu 1.165e-2 (ratios 1.07 and 1.12; profiles/decode/README.md)."""
    torch.manual_seed(0)
    cfg = get_preset(preset, seq_len=128, **over)
    m32 = Transformer(cfg).eval()
    m16 = Transformer(cfg)
    m16.load_state_dict(m32.state_dict())
    m16 = m16.bfloat16().eval()
    m32.load_state_dict(m16.state_dict())  # the same (bf16-representable) weights in fp32
    mg = Transformer(cfg).to(cuda)
    mg.load_state_dict(m16.state_dict())
    mg = mg.bfloat16().eval()
    B, P, N = 2, 64, 32
    tok = torch.randint(0, cfg.vocab_size, (B, P + N))
    ref = _teacher_forced(m32, tok, P, N, torch.float32, "cpu")
    cpu = _teacher_forced(m16, tok, P, N, torch.bfloat16, "cpu")
    gpu = _teacher_forced(mg, tok.to(cuda), P, N, torch.bfloat16, cuda)
    e_ref, e_gpu = (cpu - ref).abs().max().item(), (gpu - ref).abs().max().item()
    print(f"e_ref = {e_ref:.3e}, e_gpu = {e_gpu:.3e}")
    assert e_gpu <= 2 * e_ref + 1e-3


PROMPTS = [[3, 4, 5, 6, 7, 8, 9], [9, 8], [1, 2, 3, 4]]  # ragged


def _micro(cuda, dtype, over, seq_len=96):
    torch.manual_seed(0)
    return Transformer(get_preset("llama-micro", seq_len=seq_len, **over)).to(cuda).to(dtype).eval()


@pytest.mark.parametrize("sampling", [dict(temperature=0.0), dict(temperature=1.1, top_k=0, top_p=0.9, seed=4)],
                         ids=["greedy", "philox"])
@pytest.mark.parametrize("dtype,over", [(torch.bfloat16, {}), (torch.float16, {"n_kv_heads": 2})],
                         ids=["bf16-gqa", "fp16-mha"])
def test_decode_graph_with_an_fp8_cache(cuda, dtype, over, sampling):
    """DecodeGraph over an fp8 cache: tokens, logits buffer and the cache's bytes and scales after N steps are
    bit-equal between eager steps and graph replays."""
    m = _micro(cuda, dtype, over)
    cfg = m.model_args
    B, N = 3, 9
    lens = torch.tensor([len(p) for p in PROMPTS], device=cuda)
    buf = torch.zeros(B, 7, dtype=torch.long, device=cuda)
    for b, p in enumerate(PROMPTS):
        buf[b, :len(p)] = torch.tensor(p)
    runs = []
    for use_graph in (False, True):
        cache = inf.KVCache(cfg, B, 48, dtype, cuda, kv_dtype="fp8")
        logits = inf.prefill(m, buf, lens, cache)
        ds = inf.DeviceSampler(lens, 48 - lens, 32, **sampling)
        if use_graph:
            dg = inf.DecodeGraph(m, cache, logits, ds)
            for _ in range(N):
                dg.step()
            assert dg.captured and dg.steps == N
            logits = dg.logits
        else:
            for _ in range(N):
                logits = inf.decode_step(m, ds.sample(logits), cache)
        runs.append((logits.clone(), ds.out.clone(), ds.count.clone(), cache.kv_len.clone(), cache._k.clone(),
                     cache._v.clone(), cache._k_scale.clone(), cache._v_scale.clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert runs[0][2].tolist() == [N] * B and runs[0][3].tolist() == (lens + N).tolist()
    assert cache._k.dtype == torch.uint8 and bool((runs[0][6][:, 0, :7] != 1).any())  # scales were written
    # generate(): graph tokens equal eager tokens, token for token
    kw = dict(sampling, sampler="philox", kv_cache_dtype="fp8")
    want, why = inf.generate(m, PROMPTS, 24, **kw)
    got, why_g = inf.generate(m, PROMPTS, 24, graph=True, **kw)
    assert got == want and why_g == why == ["max_new_tokens"] * 3


def test_generate_py_fp8_cache_from_a_train_py_checkpoint(cuda, tmp_path):
    """train.py writes a checkpoint; generate.py --kv-cache-dtype fp8 runs from it on the HIP decode path, the
    JSONL records the dtype, and the first generated token of each prompt equals that of the model-dtype cache
    (computed in this process from the same checkpoint)."""
    from pyrecover_amd.ckpt.model_only import load_model_only

    train = [sys.executable, os.path.join(ROOT, "train.py"), "--model-preset", "llama-micro", "--synthetic-data",
             "--batch-size", "2", "--sequence-length", "128", "--training-steps", "2", "--checkpoint-frequency", "2",
             "--logging-frequency", "1", "--num-workers", "0", "--checkpoint-dir", str(tmp_path),
             "--experiment_name", "gen"]
    r = subprocess.run(train, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    out = tmp_path / "fp8.jsonl"
    gen = [sys.executable, os.path.join(ROOT, "generate.py"), "--model-preset", "llama-micro", "--sequence-length",
           "128", "--checkpoint-dir", str(tmp_path), "--prompt-tokens", "3,4,5", "--prompt-tokens", "9,8,7,6,5,4,3",
           "--max-new-tokens", "20", "--kv-cache-dtype", "fp8", "--output-jsonl", str(out)]
    r = subprocess.run(gen, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "runs PyTorch math" not in r.stderr  # the HIP kernels ran
    recs = [json.loads(line) for line in out.read_text().splitlines()]
    assert [x["kv_cache_dtype"] for x in recs] == ["fp8", "fp8"]
    assert [len(x["generated_ids"]) for x in recs] == [20, 20]
    assert all(x["finish_reason"] == "max_new_tokens" and x["decode_ms_per_token"] > 0 for x in recs)
    from pyrecover_amd.cli import PRECISION_STR_TO_DTYPE
    from pyrecover_amd.generate import build_parser

    dtype = PRECISION_STR_TO_DTYPE[build_parser().get_default("model_dtype")]
    m = Transformer(get_preset("llama-micro", seq_len=128)).to(cuda).to(dtype).eval()
    load_model_only(m, str(tmp_path))
    m.flatten_(shadows=False)
    want, _ = inf.generate(m, [[3, 4, 5], [9, 8, 7, 6, 5, 4, 3]], 20)
    assert [x["generated_ids"][0] for x in recs] == [t[0] for t in want]
