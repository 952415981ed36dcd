"""MXFP4 KV cache on the GPU (csrc/kernels/attention_decode_fp4.hip): stores against the table oracle, attn_decode_fp4
against the fp64 oracle on the dequantized cache, its bit contracts, the bindings' checks, the model level."""
import pytest
import torch

from pyrecover_amd import _ext
from pyrecover_amd import inference as inf
from pyrecover_amd.config import get_preset
from pyrecover_amd.models.llama import Transformer
from pyrecover_amd.ops import reference as R
from tests import attention_oracles as A
from tests import kv_fp4_oracles as Q
from tests.kv_fp8_oracles import GROUPS, RECIPES
from tests.test_attention_rowerr_gpu import Judge

pytestmark = pytest.mark.gpu
DTYPES = (torch.bfloat16, torch.float16)
HEADS = [(4, 4), (8, 2), (8, 1)]
BYTE, SCALE = 0xAB, 77  # what an untouched cache row and scale byte hold in the store tests


def _lens(cuda, lens):
    return torch.tensor(lens, device=cuda, dtype=torch.int32)


def _caches(cuda, B, cap, Hkv, D, byte=BYTE, scale=SCALE):
    kq = torch.full((B, cap, Hkv, D // 2), byte, dtype=torch.uint8, device=cuda)
    ks = torch.full((B, cap, Hkv, D // 32), scale, dtype=torch.uint8, device=cuda)
    return kq, kq.clone(), ks, ks.clone()


def _activation(cuda, rows, Hq, Hkv, D, dtype, edge_every):
    """A strided fused QKV activation whose k and v parts of every ``edge_every``-th row carry the rule's edge rows."""
    nq, nk = Hq * D, Hkv * D
    act = (torch.randn(rows, nq + 2 * nk, generator=torch.Generator().manual_seed(0)) * 3).to(dtype)
    edges = Q.edge_rows(dtype, D)
    for i, r in enumerate(range(0, rows, edge_every)):
        pick = edges[(torch.arange(2 * Hkv) + 2 * Hkv * i) % len(edges)]
        act[r, nq:] = pick.reshape(2 * nk)
    base = torch.zeros(rows, nq + 2 * nk + 24, dtype=dtype, device=cuda)
    base[:, :nq + 2 * nk] = act
    return base[:, :nq + 2 * nk], act.to(cuda)


@pytest.mark.parametrize("dtype", DTYPES, ids=A.dname)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_kv_quantize_fp4_bits(cuda, Hq, Hkv, D, dtype):
    """Rows 0 .. S - 1 bit-equal to the oracle, the other rows and scale bytes untouched, the activation read only."""
    C = _ext.native()
    B, S, cap = 3, 7, 10
    nq, nk = Hq * D, Hkv * D
    qkv, act = _activation(cuda, B * S, Hq, Hkv, D, dtype, 2)
    k, v = qkv[:, nq:nq + nk].view(B, S, Hkv, D), qkv[:, nq + nk:].view(B, S, Hkv, D)
    kq, vq, ks, vs = _caches(cuda, B, cap, Hkv, D)
    C.kv_quantize_fp4_(k, v, kq, vq, ks, vs)
    for x, q, s in ((k, kq, ks), (v, vq, vs)):
        wq, ws = Q.quantize(x.cpu())
        assert torch.equal(q[:, :S].cpu(), wq) and torch.equal(s[:, :S].cpu(), ws)
        assert bool((q[:, S:] == BYTE).all()) and bool((s[:, S:] == SCALE).all())
    assert torch.equal(qkv, act)


ROPE_CASES = [(Hq, Hkv, D, T, 6, dt) for Hq, Hkv in HEADS for D in (64, 128) for T in (1, 3) for dt in DTYPES]
ROPE_CASES.append((4, 4, 128, 1, 2731, torch.bfloat16))  # 524352 work items > one pass of the grid, 2048 * 256


@pytest.mark.parametrize("Hq,Hkv,D,T,B,dtype", ROPE_CASES, ids=lambda v: A.dname(v) if isinstance(v, torch.dtype) else str(v))
def test_rope_append_fp4_bits(cuda, Hq, Hkv, D, T, B, dtype):
    """q bit-equal to rope_append_'s; every cache row is the oracle applied to the row rope_append_ writes into a
    16-bit cache (same rows, same overflow rule), all other rows and scale bytes untouched. Even sequences sit at
    position 0, where the rotation is the identity and the edge rows reach the store as they are."""
    C = _ext.native()
    cap = 12
    tab = R.rope_table(R.precompute_freqs_cis(D, cap)).to(cuda)
    qkv, act = _activation(cuda, B * T, Hq, Hkv, D, dtype, 2 * T)
    n = _lens(cuda, [(0, 5, 0, cap - 1, 0, cap + 9, 0, -2)[b % 8] for b in range(B)])
    kc16, vc16 = (torch.zeros(B, cap, Hkv, D, dtype=dtype, device=cuda) for _ in range(2))
    written = torch.zeros(B, cap, Hkv, D, dtype=dtype, device=cuda)
    C.rope_append_(act, tab, n, kc16, vc16)  # act: now the 16-bit path's q
    C.rope_append_(torch.ones_like(act), tab, n, written.clone(), written)  # v rows of ones mark what is stored
    kq, vq, ks, vs = _caches(cuda, B, cap, Hkv, D)
    C.rope_append_fp4_(qkv, tab, n, kq, vq, ks, vs)
    assert torch.equal(qkv, act)
    rows = (written != 0).any(-1).any(-1).cpu()  # [B, cap]: the rows the 16-bit append stored
    assert int(rows.sum()) >= B
    for x16, q, s in ((kc16, kq, ks), (vc16, vq, vs)):
        wq, ws = Q.quantize(x16.cpu())
        q, s = q.cpu(), s.cpu()
        assert torch.equal(q[rows], wq[rows]) and torch.equal(s[rows], ws[rows])
        assert bool((q[~rows] == BYTE).all()) and bool((s[~rows] == SCALE).all())


def _case_dev(c, cuda):
    return [t.to(cuda) for t in (c.q[:, 0], c.kq, c.vq, c.ks, c.vs, c.kv_len)]


@pytest.mark.parametrize("dtype", DTYPES, ids=A.dname)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Hq,Hkv", GROUPS)
def test_attn_decode_fp4_row_error(cuda, Hq, Hkv, D, dtype):
    """rho <= cap(dtype, "decode_o") = 2 u, lse within lse_bound, two runs bit-equal. The cap is derived: dequantization
    is exact, the scales are powers of two, P and the partials stay fp32; the only 16-bit rounding is the store of o."""
    C = _ext.native()
    KC = C.attn_decode_fp4_chunk()
    J = Judge("decode_fp4")
    for name in RECIPES:
        c = Q.decode_case(name, D, dtype, Hq, Hkv, KC)
        assert c.kv_len.tolist() == [1, KC - 1, KC, KC + 1, 3 * KC + 17]
        args = _case_dev(c, cuda)
        o, lse = C.attn_decode_fp4(*args, c.scale)
        assert o.dtype == dtype and lse.dtype == torch.float32
        J.same(c, "decode_fp4", (o, lse), C.attn_decode_fp4(*args, c.scale))
        J.row(c, "decode_fp4", "o", o[:, None], c.o, c.m_o, A.cap(dtype, "decode_o"))
        J.lse(c, "decode_fp4", lse[:, :, None])
    J.done()


@pytest.mark.parametrize("D,Hq,Hkv", [(128, 8, 1), (64, 4, 2)])
def test_attn_decode_fp4_depends_on_own_data_only(cuda, D, Hq, Hkv):
    """A sequence's output is a function of its own data: alone or in a ragged batch, at another cap, whatever the cache
    holds at and beyond kv_len (scale bytes 0xFF, any nibbles); length 0 gives o = 0, lse = -inf; lengths clamp."""
    C = _ext.native()
    KC = C.attn_decode_fp4_chunk()
    c = Q.decode_case("peaked", D, torch.bfloat16, Hq, Hkv, KC)
    q, kq, vq, ks, vs, _ = _case_dev(c, cuda)
    L = 2 * KC + 3
    o, lse = C.attn_decode_fp4(q, kq, vq, ks, vs, _lens(cuda, [KC + 1, L, 1, 0, KC]), c.scale)
    assert torch.equal(o[3], torch.zeros_like(o[3])) and bool(torch.isneginf(lse[3]).all())
    assert bool(torch.isfinite(o).all()) and bool(torch.isfinite(lse[[0, 1, 2, 4]]).all())
    q1 = q[1:2].contiguous()
    for byte, scale in ((0, 127), (0xF7, 0xFF), (0x9E, 0)):  # a larger cache: zero tail, poisoned tails
        kb, vb, sk, sv = _caches(cuda, 1, 4 * KC + 64, Hkv, D, byte, scale)
        kb[0, :L], vb[0, :L], sk[0, :L], sv[0, :L] = kq[1, :L], vq[1, :L], ks[1, :L], vs[1, :L]
        ob, lb = C.attn_decode_fp4(q1, kb, vb, sk, sv, _lens(cuda, [L]), c.scale)
        assert torch.equal(ob[0], o[1]) and torch.equal(lb[0], lse[1])
    cap = kq.shape[1]
    a = C.attn_decode_fp4(q, kq, vq, ks, vs, _lens(cuda, [-3, 0, cap + 5, 1, 2]), c.scale)
    b = C.attn_decode_fp4(q, kq, vq, ks, vs, _lens(cuda, [0, 0, cap, 1, 2]), c.scale)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_fp4_bindings_reject_bad_arguments(cuda):
    C = _ext.native()
    D, Hq, Hkv, cap, B = 64, 4, 2, 32, 2
    q = torch.randn(B, Hq, D, device=cuda).bfloat16()
    kq, vq, ks, vs = _caches(cuda, B, cap, Hkv, D)
    n = _lens(cuda, [3, 4])
    tab = R.rope_table(R.precompute_freqs_cis(D, cap)).to(cuda)
    qkv = torch.randn(B, (Hq + 2 * Hkv) * D, device=cuda).bfloat16()
    k16 = torch.randn(B, 4, Hkv, D, device=cuda).bfloat16()
    q96 = torch.randn(B, Hq, 96, device=cuda).bfloat16()
    C.attn_decode_fp4(q, kq, vq, ks, vs, n, 0.125)  # the good calls
    C.rope_append_fp4_(qkv.clone(), tab, n, kq, vq, ks, vs)
    C.kv_quantize_fp4_(k16, k16, kq, vq, ks, vs)
    bad = [("bf16 or fp16", lambda: C.attn_decode_fp4(q.float(), kq, vq, ks, vs, n, 0.125)),
           ("uint8", lambda: C.attn_decode_fp4(q, kq.bfloat16(), vq.bfloat16(), ks, vs, n, 0.125)),
           ("k_scale and v_scale", lambda: C.attn_decode_fp4(q, kq, vq, ks[..., :1].contiguous(), vs, n, 0.125)),
           ("must be on", lambda: C.attn_decode_fp4(q, kq, vq.cpu(), ks, vs, n, 0.125)),
           ("head_dim", lambda: C.attn_decode_fp4(q96, *_caches(cuda, B, cap, Hkv, 96), n, 0.1)),
           ("disagree on head_dim", lambda: C.attn_decode_fp4(q.repeat(1, 1, 2), kq, vq, ks, vs, n, 0.1)),
           ("bf16 or fp16", lambda: C.rope_append_fp4_(qkv.float(), tab, n, kq, vq, ks, vs)),
           ("qkv must be", lambda: C.rope_append_fp4_(qkv[:, :-D].contiguous(), tab, n, kq, vq, ks, vs)),
           ("do not fit", lambda: C.kv_quantize_fp4_(k16.repeat(1, 9, 1, 1), k16.repeat(1, 9, 1, 1), kq, vq, ks, vs)),
           ("v must have", lambda: C.kv_quantize_fp4_(k16, k16.half(), kq, vq, ks, vs))]
    for match, call in bad:
        with pytest.raises(RuntimeError, match=match):
            call()


def _teacher_forced(m, tok, P, N, dtype, dev, kv_dtype):
    cache = inf.KVCache(m.model_args, tok.shape[0], P + N, dtype, dev, kv_dtype=kv_dtype)
    rows = [inf.prefill(m, tok[:, :P], torch.full((tok.shape[0],), P, device=dev), cache)]
    rows += [inf.decode_step(m, tok[:, t], cache) for t in range(P, P + N - 1)]
    return torch.stack(rows, 1).double().cpu()


@pytest.mark.parametrize("over", [{}, {"dim": 512, "n_heads": 4, "n_kv_heads": 1}], ids=["micro", "d128-gqa4"])
def test_decode_logits_fp4_cache_vs_fp64_reference(cuda, over):
    """Teacher-forced, 24-token prefill then 15 decode steps: bf16 HIP logits against the fp64 torch-math path on the
    CPU with the same weights, tokens and kind of cache. The bound is the same comparison for the fp8 cache in this
    run: e_fp4 <= 2 * e_fp8 (same numerics, only the stored values differ). Measured on MI355X: micro e_fp8 1.022e-2,
    e_fp4 1.134e-2; head_dim 128, GQA 4:1 e_fp8 1.018e-2, e_fp4 1.283e-2 (profiles/decode/README.md)."""
    torch.manual_seed(0)
    cfg = get_preset("llama-micro", seq_len=64, **over)
    m64 = Transformer(cfg).bfloat16().double().eval()  # bf16-representable weights
    mg = Transformer(cfg).to(cuda)
    mg.load_state_dict(m64.state_dict())
    mg = mg.bfloat16().eval()
    tok = torch.randint(0, cfg.vocab_size, (2, 40))
    e = {}
    for kind in ("fp8", "fp4"):
        ref = _teacher_forced(m64, tok, 24, 16, torch.float64, "cpu", kind)
        e[kind] = (_teacher_forced(mg, tok.to(cuda), 24, 16, torch.bfloat16, cuda, kind) - ref).abs().max().item()
    print(f"e_fp8 = {e['fp8']:.3e}, e_fp4 = {e['fp4']:.3e}")
    assert e["fp4"] <= 2 * e["fp8"]


@pytest.mark.parametrize("dtype,over", [(torch.bfloat16, {}), (torch.float16, {"n_kv_heads": 2})], ids=["bf16-gqa", "fp16-mha"])
def test_generate_fp4_plain_and_graph(cuda, dtype, over):
    torch.manual_seed(0)
    m = Transformer(get_preset("llama-micro", seq_len=96, **over)).to(cuda).to(dtype).eval()
    prompts = [[3, 4, 5, 6, 7, 8, 9], [9, 8], [1, 2, 3, 4]]
    kw = dict(temperature=1.1, top_p=0.9, seed=4, sampler="philox", kv_cache_dtype="fp4")
    want, why = inf.generate(m, prompts, 24, **kw)
    got, why_g = inf.generate(m, prompts, 24, graph=True, **kw)
    assert got == want and why_g == why == ["max_new_tokens"] * 3
    first = [t[0] for t in inf.generate(m, prompts, 1, **dict(kw, kv_cache_dtype="model"))[0]]
    assert [t[0] for t in want] == first  # the prompt's attention is unquantized
