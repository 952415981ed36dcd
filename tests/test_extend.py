"""Multi-token KV-cache append on the CPU (torch-math path of pyrecover_amd.inference): the oracle of the
extend kernel against causal attention, ``extend`` / chunked ``prefill`` against the one-shot prefill and
``decode_step`` in fp64, the fp8 refusal, and generate.py --prefill-chunk end to end."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

from pyrecover_amd import inference as inf
from pyrecover_amd.config import get_preset
from pyrecover_amd.models.llama import Transformer
from pyrecover_amd.ops import reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-9


def _model(preset="llama-micro", seq_len=64, seed=0, dtype=torch.float64, **kw):
    torch.manual_seed(seed)
    return Transformer(get_preset(preset, seq_len=seq_len, **kw)).to(dtype).eval()


def _qkv(B, S, hq, hkv, D, seed=0):
    torch.manual_seed(seed)
    return tuple(torch.randn(B, S, h, D, dtype=torch.float64) for h in (hq, hkv, hkv))


def _poisoned(k, v, cap):
    """Caches of capacity ``cap`` that hold k / v in rows 0 .. S - 1 and NaN / Inf beyond."""
    B, S, hkv, D = k.shape
    kc = torch.full((B, cap, hkv, D), float("nan"), dtype=k.dtype)
    vc = torch.full((B, cap, hkv, D), float("inf"), dtype=k.dtype)
    kc[:, :S], vc[:, :S] = k, v
    return kc, vc


# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("hq,hkv", [(4, 4), (8, 2)])
def test_attention_extend_ref_on_an_empty_cache_is_causal_attention(hq, hkv):
    B, S, D = 2, 19, 16
    q, k, v = _qkv(B, S, hq, hkv, D)
    kc, vc = _poisoned(k, v, S + 5)
    o, lse = ref.attention_extend_ref(q, kc, vc, torch.tensor([0, 0]), 1 / math.sqrt(D))
    _, lse_all = ref.attention_lse_ref(q, k, v, causal=True)
    assert (o - ref.attention_ref(q, k, v, causal=True)).abs().max().item() < 1e-12
    assert (lse - lse_all.transpose(1, 2)).abs().max().item() < 1e-12  # [B, T, Hq] against [B, Hq, S]


@pytest.mark.parametrize("hq,hkv", [(4, 4), (8, 2)])
def test_attention_extend_ref_single_token_is_attention_decode_ref(hq, hkv):
    B, S, D = 3, 19, 16
    q, k, v = _qkv(B, S, hq, hkv, D, seed=1)
    kc, vc = _poisoned(k, v, S)
    n = torch.tensor([0, 7, S - 1])
    o, lse = ref.attention_extend_ref(q[:, :1], kc, vc, n, 1 / math.sqrt(D))
    od, lsed = ref.attention_decode_ref(q[:, 0], kc, vc, n + 1, 1 / math.sqrt(D))
    assert (o[:, 0] - od).abs().max().item() < 1e-12 and (lse[:, 0] - lsed).abs().max().item() < 1e-12


@pytest.mark.parametrize("hq,hkv", [(4, 4), (8, 2)])
def test_attention_extend_ref_ragged_is_causal_attention_over_the_concatenation(hq, hkv):
    """Sequence b holds n[b] keys and appends T: row t is row n[b] + t of causal attention over n[b] + T."""
    B, T, D = 3, 6, 16
    n = [0, 5, 11]
    cap = max(n) + T + 3
    q, _, _ = _qkv(B, T, hq, hkv, D, seed=2)
    _, k, v = _qkv(B, cap, hq, hkv, D, seed=3)
    kc, vc = k.clone(), v.clone()
    for b in range(B):
        kc[b, n[b] + T:], vc[b, n[b] + T:] = float("nan"), float("-inf")
    o, lse = ref.attention_extend_ref(q, kc, vc, torch.tensor(n), 1 / math.sqrt(D))
    for b in range(B):
        L = n[b] + T
        qq = torch.zeros(1, L, hq, D, dtype=torch.float64)
        qq[0, n[b]:] = q[b]
        want, lse_w = ref.attention_lse_ref(qq, k[b:b + 1, :L], v[b:b + 1, :L], causal=True)
        assert (o[b] - want[0, n[b]:]).abs().max().item() < 1e-12, b
        assert (lse[b] - lse_w[0, :, n[b]:].t()).abs().max().item() < 1e-12, b


def test_attention_extend_ref_clamps_to_the_capacity():
    """kv_len outside [0, cap] clamps into it, and a query at or beyond the capacity sees keys 0 .. cap - 1."""
    B, T, cap, H, D = 3, 4, 9, 2, 8
    q, _, _ = _qkv(B, T, H, H, D)
    _, kc, vc = _qkv(B, cap, H, H, D, seed=1)
    o, lse = ref.attention_extend_ref(q, kc, vc, torch.tensor([-3, cap + 5, cap - 2]))
    oc, lsec = ref.attention_extend_ref(q, kc, vc, torch.tensor([0, cap, cap - 2]))
    assert torch.equal(o, oc) and torch.equal(lse, lsec) and torch.isfinite(o).all()
    full, _ = ref.attention_decode_ref(q[:, -1], kc, vc, torch.tensor([cap] * B))
    assert (o[1:, -1] - full[1:]).abs().max().item() < 1e-12  # rows at positions cap + 3 and cap + 1


def test_rope_append_ref_multi_token_matches_rope_inplace():
    """Row b * T + t is rotated with table row kv_len[b] + t and stored there; past the capacity nothing is
    stored and q takes table row cap - 1; every other cache row is untouched."""
    torch.manual_seed(0)
    B, T, cap, Hq, Hkv, D = 3, 4, 12, 4, 2, 8
    tab = ref.rope_table(ref.precompute_freqs_cis(D, cap))
    qkv = torch.randn(B * T, (Hq + 2 * Hkv) * D, dtype=torch.float64)
    kc, vc = torch.randn(B, cap, Hkv, D, dtype=torch.float64), torch.randn(B, cap, Hkv, D, dtype=torch.float64)
    kc0, vc0 = kc.clone(), vc.clone()
    base = [0, cap - T, cap - 2]  # the last one runs two rows past the capacity
    nq, nk = Hq * D, Hkv * D
    want = qkv.clone()
    for b in range(B):
        for t in range(T):
            p = min(base[b] + t, cap - 1)
            row = want[b * T + t:b * T + t + 1].repeat(p + 1, 1)
            ref.rope_inplace_2d(row, nq + nk, tab, D, p + 1)
            want[b * T + t] = row[p]
    got = qkv.clone()
    ref.rope_append_ref(got, tab, torch.tensor(base), kc, vc)
    assert torch.equal(got[:, :nq], want[:, :nq]) and torch.equal(got[:, nq:], qkv[:, nq:])
    for b in range(B):
        for t in range(T):
            p = base[b] + t
            if p < cap:
                assert torch.equal(kc[b, p].reshape(-1), want[b * T + t, nq:nq + nk])
                assert torch.equal(vc[b, p].reshape(-1), qkv[b * T + t, nq + nk:])
                kc0[b, p], vc0[b, p] = kc[b, p], vc[b, p]
    assert torch.equal(kc, kc0) and torch.equal(vc, vc0)


# ---------------------------------------------------------------------------------------
def _ragged(m, lens, extra, seed):
    """Per sequence lens[b] + extra[b] tokens; the right-padded prompt [B, max lens] and append [B, max extra]."""
    g = torch.Generator().manual_seed(seed)
    seqs = [torch.randint(0, m.vocab_size, (p + e,), generator=g) for p, e in zip(lens, extra)]
    prompt = torch.zeros(len(lens), max(lens), dtype=torch.long)
    app = torch.zeros(len(lens), max(extra), dtype=torch.long)
    for b, s in enumerate(seqs):
        prompt[b, :lens[b]] = s[:lens[b]]
        app[b, :extra[b]] = s[lens[b]:]
    return seqs, prompt, app


@pytest.mark.parametrize("preset", ["llama-micro", "llama-tiny"])
@pytest.mark.parametrize("lens,extra", [([8, 8], [6, 6]), ([3, 8], [6, 6]), ([8, 5], [7, 2]), ([1, 4], [1, 9])])
def test_prefill_then_extend_equals_prefill_of_both(preset, lens, extra):
    """prefill(p) + extend(t) against prefill(p + t): the logits and every cache row below the new kv_len."""
    m = _model(preset)
    seqs, prompt, app = _ragged(m, lens, extra, seed=1)
    B, cap = len(lens), 24
    tot = [p + e for p, e in zip(lens, extra)]
    both = torch.zeros(B, max(tot), dtype=torch.long)
    for b, s in enumerate(seqs):
        both[b, :tot[b]] = s
    want_cache = inf.KVCache(m.model_args, B, cap, torch.float64, "cpu")
    want = inf.prefill(m, both, torch.tensor(tot), want_cache)
    cache = inf.KVCache(m.model_args, B, cap, torch.float64, "cpu")
    inf.prefill(m, prompt, torch.tensor(lens), cache)
    got = inf.extend(m, app, torch.tensor(extra), cache)
    assert got.shape == want.shape and (got - want).abs().max().item() < TOL
    assert cache.kv_len.tolist() == tot == want_cache.kv_len.tolist()
    for i in range(len(cache.k)):
        for b in range(B):
            assert (cache.k[i][b, :tot[b]] - want_cache.k[i][b, :tot[b]]).abs().max().item() < TOL
            assert (cache.v[i][b, :tot[b]] - want_cache.v[i][b, :tot[b]]).abs().max().item() < TOL
    # every row's logits, against the full forward of each sequence
    cache2 = inf.KVCache(m.model_args, B, cap, torch.float64, "cpu")
    inf.prefill(m, prompt, torch.tensor(lens), cache2)
    rows = inf.extend(m, app, torch.tensor(extra), cache2, return_all=True)
    assert rows.shape == (B, max(extra), m.vocab_size)
    with torch.no_grad():
        for b, s in enumerate(seqs):
            full = m(s[None])[0]
            assert (rows[b, :extra[b]] - full[lens[b]:]).abs().max().item() < TOL


@pytest.mark.parametrize("lens", [[11, 11], [11, 4]])
@pytest.mark.parametrize("chunk", [1, 5, 11, 14])
def test_chunked_prefill_equals_prefill(lens, chunk):
    """chunk in {1, 5, S, S + 3} at S = 11: logits, kv_len and the cache rows of the one-shot prefill."""
    m = _model("llama-tiny")
    S = 11
    _, prompt, _ = _ragged(m, lens, [1, 1], seed=2)
    want_cache = inf.KVCache(m.model_args, 2, 16, torch.float64, "cpu")
    want = inf.prefill(m, prompt, torch.tensor(lens), want_cache)
    cache = inf.KVCache(m.model_args, 2, 16, torch.float64, "cpu")
    got = inf.prefill(m, prompt, torch.tensor(lens), cache, chunk=chunk)
    assert (got - want).abs().max().item() < TOL
    assert cache.kv_len.tolist() == lens == want_cache.kv_len.tolist()
    for i in range(len(cache.k)):
        assert (cache.k[i][:, :S] - want_cache.k[i][:, :S]).abs().max().item() < TOL
        assert (cache.v[i][:, :S] - want_cache.v[i][:, :S]).abs().max().item() < TOL


@pytest.mark.parametrize("preset", ["llama-micro", "llama-tiny"])
def test_extend_single_token_equals_decode_step(preset):
    m = _model(preset)
    _, prompt, app = _ragged(m, [3, 8], [5, 5], seed=3)
    caches = [inf.KVCache(m.model_args, 2, 12, torch.float64, "cpu") for _ in range(2)]
    for c in caches:
        inf.prefill(m, prompt, torch.tensor([3, 8]), c)
    for t in range(5):  # the last step of sequence 1 finds the cache full: both overwrite the last row
        a = inf.decode_step(m, app[:, t], caches[0])
        b = inf.extend(m, app[:, t:t + 1], torch.tensor([1, 1]), caches[1])
        assert (a - b).abs().max().item() < TOL, t
        assert caches[0].kv_len.tolist() == caches[1].kv_len.tolist()
    assert caches[1].kv_len.tolist() == [8, 12]
    for i in range(len(caches[0].k)):
        assert (caches[0].k[i] - caches[1].k[i]).abs().max().item() < TOL
        assert (caches[0].v[i] - caches[1].v[i]).abs().max().item() < TOL


def test_extend_past_the_capacity_clamps():
    """Tokens at or beyond the capacity store nothing, leave the rows below untouched, and kv_len stops at
    the capacity; everything stays finite."""
    m = _model("llama-micro")
    _, prompt, app = _ragged(m, [6, 6], [5, 5], seed=4)
    cache = inf.KVCache(m.model_args, 2, 8, torch.float64, "cpu")
    inf.prefill(m, prompt, torch.tensor([6, 6]), cache)
    k0 = [k.clone() for k in cache.k]
    out = inf.extend(m, app, torch.tensor([5, 2]), cache, return_all=True)
    assert torch.isfinite(out).all() and cache.kv_len.tolist() == [8, 8]
    for i in range(len(cache.k)):
        assert torch.equal(cache.k[i][:, :6], k0[i][:, :6])
    # the two tokens that fit are those of an append that fits
    fit = inf.KVCache(m.model_args, 2, 8, torch.float64, "cpu")
    inf.prefill(m, prompt, torch.tensor([6, 6]), fit)
    want = inf.extend(m, app[:, :2], torch.tensor([2, 2]), fit, return_all=True)
    assert (out[:, :2] - want).abs().max().item() < TOL


def test_generate_with_chunked_prefill_gives_the_greedy_tokens():
    m = _model("llama-tiny")
    prompts = [[5, 9, 2], [7, 1, 4, 4, 8, 3, 11, 6, 2, 9]]
    stats_a, stats_b = {}, {}
    a, ra = inf.generate(m, prompts, 16, stats=stats_a)
    b, rb = inf.generate(m, prompts, 16, prefill_chunk=4, stats=stats_b)
    assert a == b and ra == rb
    assert stats_a["prefill_chunks"] == 0 and stats_b["prefill_chunks"] == 3
    with pytest.raises(ValueError, match="prefill_chunk"):
        inf.generate(m, prompts, 4, prefill_chunk=4, use_cache=False)


def test_extend_refuses_an_fp8_cache():
    m = _model("llama-micro", dtype=torch.float32)
    cache = inf.KVCache(m.model_args, 2, 16, torch.float32, "cpu", kv_dtype="fp8")
    tok = torch.tensor([[3, 4, 5], [9, 8, 7]])
    with pytest.raises(ValueError, match="fp8"):
        inf.prefill(m, tok, torch.tensor([3, 3]), cache, chunk=2)
    inf.prefill(m, tok, torch.tensor([3, 3]), cache)  # the one-shot prefill serves it
    with pytest.raises(ValueError, match="fp8"):
        inf.extend(m, tok, torch.tensor([3, 3]), cache)
    with pytest.raises(ValueError, match="fp8"):
        inf.generate(m, [[3, 4, 5]], 4, kv_cache_dtype="fp8", prefill_chunk=2)


# ---------------------------------------------------------------------------------------
def _trained(tmp_path):
    from pyrecover_amd.ckpt import core
    from pyrecover_amd.ckpt.vanilla import save_ckpt_vanilla
    from pyrecover_amd.optim.adamw import FlatAdamW
    from pyrecover_amd.optim.lr import build_lr_scheduler

    torch.manual_seed(0)
    m = Transformer(get_preset("llama-micro", seq_len=32))
    opt = FlatAdamW(m.flatten_(), lr=1e-2)
    sched = build_lr_scheduler(opt, 2)
    g = torch.Generator().manual_seed(5)
    for _ in range(2):
        t = torch.randint(0, m.vocab_size, (2, 33), generator=g)
        opt.zero_grad()
        m(t[:, :-1], labels=t[:, 1:]).backward()
        opt.step()
        sched.step()
    exp = tmp_path / "exp"
    exp.mkdir()
    save_ckpt_vanilla(m, opt, sched, None, 2, 1, str(exp / "ckpt_2.pt"), max_keep=0, verify=True)
    core.wait_all()


def test_generate_cli_prefill_chunk_round_trip(tmp_path):
    from pyrecover_amd import _ext

    if not _ext.available():
        pytest.skip("native extension not built (the checkpoint writer is native)")
    _trained(tmp_path)
    common = [sys.executable, os.path.join(ROOT, "generate.py"), "--checkpoint-dir", str(tmp_path), "--model-preset",
              "llama-micro", "--sequence-length", "32", "--model-dtype", "fp64", "--prompt-tokens", "3,4,5",
              "--prompt-tokens", "9,8,7,6,5,4,3,2,1", "--max-new-tokens", "8"]
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    outs = []
    for extra, name, pieces in (([], "a.jsonl", 0), (["--prefill-chunk", "4"], "b.jsonl", 3),
                                (["--prefill-chunk", "512"], "c.jsonl", 1)):
        out = tmp_path / name
        r = subprocess.run(common + extra + ["--output-jsonl", str(out)], capture_output=True, text=True, env=env,
                           timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        recs = [json.loads(line) for line in out.read_text().splitlines()]
        assert len(recs) == 2 and all(rec["prefill_chunks"] == pieces for rec in recs)
        assert all(len(rec["generated_ids"]) == 8 for rec in recs)
        outs.append([rec["generated_ids"] for rec in recs])
    assert outs[0] == outs[1] == outs[2]
