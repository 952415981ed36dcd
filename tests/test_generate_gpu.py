"""KV-cache generation on the GPU: the decode kernels (csrc/kernels/attention_decode.hip) against the
torch oracle and against their own bit-reproducibility contract, the model-level decode path against
the fp32 plain-torch model, and generate.py from a train.py checkpoint."""
import json
import math
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

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# bounds of test_kernels_gpu.py::test_attention_fwd
O_TOL, LSE_TOL = 2e-2, 1e-3


def _kc():
    return _ext.native().attn_decode_chunk()


def _inputs(cuda, B, cap, Hq, Hkv, D, dtype, seed=0):
    """Standard normal q and caches, as _qkv of the kernel tests makes them."""
    torch.manual_seed(seed)
    q = torch.randn(B, Hq, D, device=cuda).to(dtype)
    k = torch.randn(B, cap, Hkv, D, device=cuda).to(dtype)
    v = torch.randn(B, cap, Hkv, D, device=cuda).to(dtype)
    return q, k, v


def _lens(cuda, lens):
    return torch.tensor(lens, device=cuda, dtype=torch.int32)


def _check(q, k, v, n, D):
    C = _ext.native()
    scale = 1 / math.sqrt(D)
    o, lse = C.attn_decode(q, k, v, n, scale)
    o_ref, lse_ref = R.attention_decode_ref(q.float(), k.float(), v.float(), n, scale)
    assert o.dtype == q.dtype and lse.dtype == torch.float32
    empty = torch.isneginf(lse_ref)  # length 0: lse = -inf on both sides (-inf - -inf is no difference)
    assert torch.equal(torch.isneginf(lse), empty)
    eo = (o.float() - o_ref).abs().max().item()
    el = (lse - lse_ref).masked_fill(empty, 0).abs().max().item()
    print(f"|o - o_ref| = {eo:.3e}, |lse - lse_ref| = {el:.3e}")
    assert eo < O_TOL and el < LSE_TOL
    return o, lse


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Hq,Hkv", [(2, 2), (4, 1), (8, 1)])
def test_attn_decode_vs_reference(cuda, dtype, D, Hq, Hkv):
    """Every edge of the chunking: lengths 1, 2, KC-1, KC, KC+1, 2KC+3, cap, and a ragged batch."""
    KC = _kc()
    cap = 4 * KC + 64
    q, k, v = _inputs(cuda, 4, cap, Hq, Hkv, D, dtype)
    _check(q, k, v, _lens(cuda, [1, 2, KC - 1, KC]), D)
    _check(q, k, v, _lens(cuda, [KC + 1, 2 * KC + 3, cap, cap]), D)
    _check(q[:3], k[:3], v[:3], _lens(cuda, [1, KC + 1, cap]), D)


@pytest.mark.parametrize("D,Hq,Hkv", [(128, 2, 2), (64, 8, 1)])
def test_attn_decode_late_score_spike(cuda, D, Hq, Hkv):
    """One huge q.k in the last chunk (as test_attention_fwd_rescale_spike): the combine step must rescale
    every earlier chunk by it."""
    KC = _kc()
    cap = 3 * KC + 40
    q, k, v = _inputs(cuda, 1, cap, Hq, Hkv, D, torch.bfloat16, seed=3)
    q[0, 0] = 4.0
    k[0, 3 * KC + 17, 0] = 4.0
    o, _ = _check(q, k, v, _lens(cuda, [cap]), D)
    # head 0 is all but that one value row
    assert (o[0, 0].float() - v[0, 3 * KC + 17, 0].float()).abs().max().item() < O_TOL


def test_attn_decode_bits(cuda):
    """Run-to-run bits, and a sequence's output as a pure function of its own q, K, V and length: alone, in
    a ragged batch, with a larger cap, and with a NaN / Inf cache tail."""
    C = _ext.native()
    KC = _kc()
    D, Hq, Hkv = 128, 8, 2
    cap = 2 * KC + 64
    scale = 1 / math.sqrt(D)
    L = 2 * KC + 3
    q, k, v = _inputs(cuda, 3, cap, Hq, Hkv, D, torch.bfloat16, seed=1)
    n = _lens(cuda, [KC + 1, L, 1])
    o, lse = C.attn_decode(q, k, v, n, scale)
    o2, lse2 = C.attn_decode(q, k, v, n, scale)
    assert torch.equal(o, o2) and torch.equal(lse, lse2)
    # sequence 1 alone
    oa, la = C.attn_decode(q[1:2].contiguous(), k[1:2].contiguous(), v[1:2].contiguous(), _lens(cuda, [L]), scale)
    assert torch.equal(oa[0], o[1]) and torch.equal(la[0], lse[1])
    # ... in a larger cache
    big = 4 * KC + 64
    kb, vb = (torch.randn(1, big, Hkv, D, device=cuda).bfloat16() for _ in range(2))
    kb[0, :L], vb[0, :L] = k[1, :L], v[1, :L]
    ob, lb = C.attn_decode(q[1:2].contiguous(), kb, vb, _lens(cuda, [L]), scale)
    assert torch.equal(ob[0], o[1]) and torch.equal(lb[0], lse[1])
    # ... with a poisoned tail against a zero tail
    kz, vz = kb.clone(), vb.clone()
    kz[0, L:], vz[0, L:] = 0, 0
    kb[0, L:L + 5], vb[0, L:L + 5] = float("nan"), float("inf")
    kb[0, L + 5:], vb[0, L + 5:] = float("-inf"), float("nan")
    op, lp = C.attn_decode(q[1:2].contiguous(), kb, vb, _lens(cuda, [L]), scale)
    oz, lz = C.attn_decode(q[1:2].contiguous(), kz, vz, _lens(cuda, [L]), scale)
    assert torch.equal(op, oz) and torch.equal(lp, lz) and torch.equal(op[0], o[1])


def test_attn_decode_clamps_kv_len(cuda):
    C = _ext.native()
    D, Hq, Hkv, cap = 64, 4, 2, 300
    scale = 1 / math.sqrt(D)
    q, k, v = _inputs(cuda, 3, cap, Hq, Hkv, D, torch.float16, seed=2)
    o, lse = C.attn_decode(q, k, v, _lens(cuda, [-3, 0, cap + 5]), scale)
    oc, lc = C.attn_decode(q, k, v, _lens(cuda, [0, 0, cap]), scale)
    assert torch.equal(o, oc) and torch.equal(lse, lc)
    assert torch.equal(o[:2], torch.zeros_like(o[:2])) and torch.isneginf(lse[:2]).all()
    assert torch.isfinite(o).all() and torch.isfinite(lse[2]).all()
    _check(q, k, v, _lens(cuda, [-3, 0, cap + 5]), D)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("D,Hq,Hkv", [(64, 4, 2), (128, 8, 1)])
def test_rope_append_bits(cuda, dtype, D, Hq, Hkv):
    """q and the cache row bit-equal to rope_ at that position, v an exact copy, every other row untouched;
    ragged positions including 0 and cap - 1."""
    C = _ext.native()
    cap, B = 40, 4
    tab = R.rope_table(R.precompute_freqs_cis(D, cap)).to(cuda)
    torch.manual_seed(0)
    qkv = torch.randn(B, (Hq + 2 * Hkv) * D, device=cuda).to(dtype)
    kc = torch.randn(B, cap, Hkv, D, device=cuda).to(dtype)
    vc = torch.randn_like(kc)
    kc0, vc0 = kc.clone(), vc.clone()
    pos = [0, cap - 1, 7, 20]
    nq, nk = Hq * D, Hkv * D
    want = qkv.clone()
    for b, p in enumerate(pos):
        C.rope_(want[b:b + 1], nq + nk, tab, D, 1, p, False, None)
    got = qkv.clone()
    C.rope_append_(got, tab, _lens(cuda, pos), kc, vc)
    assert torch.equal(got[:, :nq], want[:, :nq])
    assert torch.equal(got[:, nq:], qkv[:, nq:])  # k and v columns of the activation stay
    for b, p in enumerate(pos):
        assert torch.equal(kc[b, p].reshape(-1), want[b, nq:nq + nk])
        assert torch.equal(vc[b, p].reshape(-1), qkv[b, nq + nk:])
        kc0[b, p], vc0[b, p] = kc[b, p], vc[b, p]
    assert torch.equal(kc, kc0) and torch.equal(vc, vc0)
    # positions outside the cache clamp into it
    kc1, vc1 = kc0.clone(), vc0.clone()
    C.rope_append_(qkv.clone(), tab, _lens(cuda, [-2, cap + 9, 7, 20]), kc1, vc1)
    assert torch.equal(kc1, kc) and torch.equal(vc1, vc)


def test_decode_bindings_reject_bad_arguments(cuda):
    C = _ext.native()
    D, Hq, Hkv, cap = 64, 4, 2, 32
    q, k, v = _inputs(cuda, 2, cap, Hq, Hkv, D, torch.bfloat16)
    n = _lens(cuda, [3, 4])
    tab = R.rope_table(R.precompute_freqs_cis(D, cap)).to(cuda)
    qkv = torch.randn(2, (Hq + 2 * Hkv) * D, device=cuda).bfloat16()
    C.attn_decode(q, k, v, n, 0.125)  # the good call
    with pytest.raises(RuntimeError, match="bf16 or fp16"):
        C.attn_decode(q.float(), k.float(), v.float(), n, 0.125)
    with pytest.raises(RuntimeError, match="dtype"):
        C.attn_decode(q, k.half(), v, n, 0.125)
    with pytest.raises(RuntimeError, match="must be on"):
        C.attn_decode(q, k.cpu(), v, n, 0.125)
    with pytest.raises(RuntimeError, match="must be on"):
        C.attn_decode(q, k, v, n.cpu(), 0.125)
    with pytest.raises(RuntimeError, match="int32"):
        C.attn_decode(q, k, v, n.long(), 0.125)
    q96, k96, v96 = _inputs(cuda, 2, cap, Hq, Hkv, 96, torch.bfloat16)
    with pytest.raises(RuntimeError, match="head_dim"):
        C.attn_decode(q96, k96, v96, n, 0.1)
    kt = torch.randn(2, Hkv, cap, D, device=cuda).bfloat16().transpose(1, 2)  # [B, cap, Hkv, D], not contiguous
    with pytest.raises(RuntimeError, match="contiguous"):
        C.attn_decode(q, kt, v, n, 0.125)
    with pytest.raises(RuntimeError, match="contiguous"):
        C.rope_append_(qkv, tab, n, kt, v)
    with pytest.raises(RuntimeError, match="bf16 or fp16"):
        C.rope_append_(qkv.float(), tab, n, k.float(), v.float())
    with pytest.raises(RuntimeError, match="must be on"):
        C.rope_append_(qkv, tab.cpu(), n, k, v)
    with pytest.raises(RuntimeError, match="table"):
        C.rope_append_(qkv, tab[:cap - 1].contiguous(), n, k, v)
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


@pytest.mark.parametrize("preset,over", [
    ("llama-tiny", {}),  # head_dim 64, GQA 2:1
    ("llama-tiny", {"dim": 512, "n_heads": 4, "n_kv_heads": 1}),  # 2 layers, head_dim 128, GQA 4:1
])
def test_decode_logits_vs_fp32_model(cuda, preset, over):
    """Teacher-forced, bf16: 64-token prefill, then 32 decode steps. With e_full / e_dec the max abs error
    of the HIP full-forward / decode-path logits against the fp32 plain-torch model on the same rows
    (63 .. 95), require e_dec <= 2 * e_full + 1e-3 (different GEMM shapes and summation orders at
    identical rounding points; the floor is for near-zero logits).

    Measured on MI355X: llama-tiny e_full 1.040e-2, e_dec 1.048e-2; head_dim-128 GQA 4:1 e_full 1.017e-2,
    e_dec 9.961e-3."""
    torch.manual_seed(0)
    cfg = get_preset(preset, seq_len=128, **over)
    m32 = Transformer(cfg).to(cuda).eval()
    m = Transformer(cfg).to(cuda)
    m.load_state_dict(m32.state_dict())
    m = m.bfloat16().eval()
    m32.load_state_dict(m.state_dict())  # the same (bf16-representable) weights in fp32
    B, P, N = 2, 64, 32
    tok = torch.randint(0, cfg.vocab_size, (B, P + N), device=cuda)
    with torch.no_grad():
        ref = _ref_forward(m32, tok)[:, P - 1:P + N - 1]
        full = m(tok).float()[:, P - 1:P + N - 1]
        cache = inf.KVCache(cfg, B, P + N, torch.bfloat16, cuda)
        rows = [inf.prefill(m, tok[:, :P], torch.full((B,), P, device=cuda), cache)]
        for t in range(P, P + N - 1):
            rows.append(inf.decode_step(m, tok[:, t], cache))
    dec = torch.stack(rows, 1).float()
    e_full, e_dec = (full - ref).abs().max().item(), (dec - ref).abs().max().item()
    print(f"e_full = {e_full:.3e}, e_dec = {e_dec:.3e}")
    assert cache.kv_len.tolist() == [P + N - 1] * B
    assert e_dec <= 2 * e_full + 1e-3


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-4), (torch.float64, 1e-9)])
def test_fp32_fp64_generate_on_torch_math_matches_cpu(cuda, dtype, tol):
    """fp32 / fp64 models on the GPU decode through attention_decode_ref / rope_append_ref."""
    torch.manual_seed(0)
    cfg = get_preset("llama-micro", seq_len=48)
    mc = Transformer(cfg).to(dtype).eval()
    mg = Transformer(cfg).to(dtype).to(cuda).eval()
    mg.load_state_dict(mc.state_dict())
    tok = torch.randint(0, cfg.vocab_size, (2, 24))
    outs = []
    for m, dev in ((mc, "cpu"), (mg, cuda)):
        cache = inf.KVCache(cfg, 2, 24, dtype, dev)
        t = tok.to(dev)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)  # the once-per-shape note of the torch-math path
            rows = [inf.prefill(m, t[:, :8], torch.tensor([8, 5]), cache)]
            rows += [inf.decode_step(m, t[:, i], cache) for i in range(8, 16)]
        outs.append(torch.stack(rows, 1).cpu())
    assert (outs[0] - outs[1]).abs().max().item() < tol
    a, ra = inf.generate(mg, [[3, 4, 5], [9, 8]], 8)
    assert all(len(x) == 8 for x in a) and ra == ["max_new_tokens"] * 2


def test_generate_py_from_a_train_py_checkpoint(cuda, tmp_path):
    """train.py writes a checkpoint (bf16 llama-micro, a few steps); generate.py samples from it on the
    HIP decode path, emits max_new_tokens ids per prompt, and the same --seed reproduces them."""
    train = [sys.executable, os.path.join(ROOT, "train.py"), "--model-preset", "llama-micro", "--synthetic-data",
             "--batch-size", "2", "--sequence-length", "128", "--training-steps", "4", "--checkpoint-frequency", "2",
             "--logging-frequency", "1", "--num-workers", "0", "--checkpoint-dir", str(tmp_path),
             "--experiment_name", "gen"]
    r = subprocess.run(train, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    gen = [sys.executable, os.path.join(ROOT, "generate.py"), "--model-preset", "llama-micro", "--sequence-length",
           "128", "--checkpoint-dir", str(tmp_path), "--prompt-tokens", "3,4,5", "--prompt-tokens", "9,8,7,6,5,4,3",
           "--max-new-tokens", "20", "--temperature", "0.8", "--top-k", "50", "--top-p", "0.95", "--seed", "11"]
    outs = []
    for name in ("a.jsonl", "b.jsonl"):
        out = tmp_path / name
        r = subprocess.run(gen + ["--output-jsonl", str(out)], capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
        assert "runs PyTorch math" not in r.stderr  # the HIP decode kernels ran
        recs = [json.loads(line) for line in out.read_text().splitlines()]
        assert [len(x["generated_ids"]) for x in recs] == [20, 20]
        assert all(x["finish_reason"] == "max_new_tokens" and 0 <= min(x["generated_ids"]) and
                   max(x["generated_ids"]) < 256 for x in recs)
        assert all(x["checkpoint_step"] == 4 and x["prefill_ms"] > 0 and x["decode_ms_per_token"] > 0 for x in recs)
        outs.append([x["generated_ids"] for x in recs])
    assert outs[0] == outs[1]
