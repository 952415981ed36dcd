"""KV-cache generation on the CPU (torch-math path of pyrecover_amd.inference): decode steps against the
full forward in fp64, the torch oracle of the decode kernels, sampling, loading only the parameters
of a checkpoint, and generate.py end to end."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

from pyrecover_amd import inference as inf
from pyrecover_amd.config import get_preset
from pyrecover_amd.data.tokenizer import ByteTokenizer
from pyrecover_amd.models.llama import Transformer
from pyrecover_amd.ops import reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(preset="llama-micro", seq_len=64, seed=0, dtype=torch.float64, **kw):
    torch.manual_seed(seed)
    return Transformer(get_preset(preset, seq_len=seq_len, **kw)).to(dtype).eval()


# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("preset", ["llama-micro", "llama-tiny"])
def test_decode_step_matches_full_forward_fp64(preset):
    """Teacher-forced over 24 positions after an 8-token prefill: the cached logits are those of the
    full forward over the prefix."""
    m = _model(preset)
    g = torch.Generator().manual_seed(1)
    toks = torch.randint(0, m.vocab_size, (2, 32), generator=g)
    with torch.no_grad():
        full = m(toks)
    cache = inf.KVCache(m.model_args, 2, 32, torch.float64, "cpu")
    logits = inf.prefill(m, toks[:, :8], torch.tensor([8, 8]), cache)
    assert (logits - full[:, 7]).abs().max().item() < 1e-9
    for t in range(8, 32):
        logits = inf.decode_step(m, toks[:, t], cache)
        assert (logits - full[:, t]).abs().max().item() < 1e-9, t
    assert cache.kv_len.tolist() == [32, 32]


@pytest.mark.parametrize("preset", ["llama-micro", "llama-tiny"])
def test_decode_step_ragged_batch_fp64(preset):
    """Prompt lengths 3 and 8 in one right-padded batch: each sequence equals its own full forward."""
    m = _model(preset)
    g = torch.Generator().manual_seed(2)
    seqs = [torch.randint(0, m.vocab_size, (3 + 24,), generator=g), torch.randint(0, m.vocab_size, (8 + 24,), generator=g)]
    lens = [3, 8]
    with torch.no_grad():
        full = [m(s[None])[0] for s in seqs]
    prompt = torch.zeros(2, 8, dtype=torch.long)
    for b in range(2):
        prompt[b, :lens[b]] = seqs[b][:lens[b]]
    cache = inf.KVCache(m.model_args, 2, 40, torch.float64, "cpu")
    logits = inf.prefill(m, prompt, torch.tensor(lens), cache)
    for b in range(2):
        assert (logits[b] - full[b][lens[b] - 1]).abs().max().item() < 1e-9
    for t in range(24):
        tok = torch.stack([seqs[b][lens[b] + t] for b in range(2)])
        logits = inf.decode_step(m, tok, cache)
        for b in range(2):
            assert (logits[b] - full[b][lens[b] + t]).abs().max().item() < 1e-9, (b, t)


def test_generate_cache_equals_naive_greedy_fp64():
    m = _model("llama-tiny")
    prompts = [[5, 9, 2], [7, 1, 4, 4, 8, 3, 11, 6]]
    a, ra = inf.generate(m, prompts, 20, use_cache=True)
    b, rb = inf.generate(m, prompts, 20, use_cache=False)
    assert a == b and ra == rb == ["max_new_tokens"] * 2
    assert all(len(x) == 20 for x in a)


def test_cache_refuses_capacity_above_seq_len():
    m = _model(seq_len=16)
    with pytest.raises(ValueError, match="seq_len"):
        inf.KVCache(m.model_args, 1, 17, torch.float64, "cpu")


# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("hq,hkv", [(4, 4), (8, 2)])
def test_attention_decode_ref_is_last_row_of_causal_attention(hq, hkv):
    torch.manual_seed(0)
    B, S, D = 2, 19, 16
    q, k, v = (torch.randn(B, S, h, D, dtype=torch.float64) for h in (hq, hkv, hkv))
    want = ref.attention_ref(q, k, v, causal=True)[:, -1]
    _, lse_all = ref.attention_lse_ref(q, k, v, causal=True)
    cap = S + 5  # rows beyond kv_len hold garbage that must not matter
    kc = torch.full((B, cap, hkv, D), float("nan"), dtype=torch.float64)
    vc = torch.full((B, cap, hkv, D), float("inf"), dtype=torch.float64)
    kc[:, :S], vc[:, :S] = k, v
    o, lse = ref.attention_decode_ref(q[:, -1], kc, vc, torch.tensor([S, S]), 1 / math.sqrt(D))
    assert (o - want).abs().max().item() < 1e-12
    assert (lse - lse_all[:, :, -1]).abs().max().item() < 1e-12
    # a shorter length is the last row of the shorter causal problem
    o2, _ = ref.attention_decode_ref(q[:, 6], kc, vc, torch.tensor([7, 7]), 1 / math.sqrt(D))
    assert (o2 - ref.attention_ref(q[:, :7], k[:, :7], v[:, :7], causal=True)[:, -1]).abs().max().item() < 1e-12


def test_attention_decode_ref_length_conventions():
    torch.manual_seed(0)
    B, cap, H, D = 3, 9, 2, 8
    q = torch.randn(B, H, D)
    kc, vc = torch.randn(B, cap, H, D), torch.randn(B, cap, H, D)
    o, lse = ref.attention_decode_ref(q, kc, vc, torch.tensor([0, -3, cap + 5]))
    assert torch.equal(o[:2], torch.zeros(2, H, D)) and torch.isneginf(lse[:2]).all()
    assert torch.isfinite(o).all()
    oc, lsec = ref.attention_decode_ref(q, kc, vc, torch.tensor([0, 0, cap]))
    assert torch.equal(o, oc) and torch.equal(lse, lsec)


def test_rope_append_ref_matches_rope_inplace():
    torch.manual_seed(0)
    B, cap, Hq, Hkv, D = 3, 12, 4, 2, 8
    tab = ref.rope_table(ref.precompute_freqs_cis(D, cap))
    qkv = torch.randn(B, (Hq + 2 * Hkv) * D, dtype=torch.float64)
    kc, vc = torch.randn(B, cap, Hkv, D, dtype=torch.float64), torch.randn(B, cap, Hkv, D, dtype=torch.float64)
    kc0, vc0 = kc.clone(), vc.clone()
    pos = [0, cap - 1, 5]
    nq, nk = Hq * D, Hkv * D
    want = qkv.clone()
    for b, p in enumerate(pos):  # one row at table position p: a length-(p + 1) sequence's last token
        row = want[b:b + 1].repeat(p + 1, 1)
        ref.rope_inplace_2d(row, nq + nk, tab, D, p + 1)
        want[b] = row[p]
    got = qkv.clone()
    ref.rope_append_ref(got, tab, torch.tensor([0, cap + 3, 5]), kc, vc)  # cap + 3 clamps to cap - 1
    assert torch.equal(got[:, :nq], want[:, :nq]) and torch.equal(got[:, nq:], qkv[:, nq:])
    for b, p in enumerate(pos):
        assert torch.equal(kc[b, p].reshape(-1), want[b, nq:nq + nk])
        assert torch.equal(vc[b, p].reshape(-1), qkv[b, nq + nk:])
        kc0[b, p], vc0[b, p] = kc[b, p], vc[b, p]
    assert torch.equal(kc, kc0) and torch.equal(vc, vc0)  # no other row touched


# ---------------------------------------------------------------------------------------
def test_sampling_seed_reproducible_and_seed_dependent():
    m = _model("llama-micro")
    prompts = [[3, 4, 5], [9, 8]]
    a, _ = inf.generate(m, prompts, 24, temperature=1.0, seed=7)
    b, _ = inf.generate(m, prompts, 24, temperature=1.0, seed=7)
    c, _ = inf.generate(m, prompts, 24, temperature=1.0, seed=8)
    assert a == b
    assert a != c


def test_top_k_one_is_greedy_and_ties_go_low():
    m = _model("llama-micro")
    prompts = [[3, 4, 5], [9, 8]]
    g, _ = inf.generate(m, prompts, 16)
    k1, _ = inf.generate(m, prompts, 16, temperature=0.9, top_k=1, seed=3)
    assert g == k1
    x = torch.tensor([[0.0, 2.0, 2.0, 1.0], [5.0, 5.0, 5.0, 5.0]])
    assert inf.greedy_token(x).tolist() == [1, 0]


def test_top_p_never_leaves_the_nucleus():
    torch.manual_seed(0)
    logits = torch.randn(4, 50, dtype=torch.float64) * 3
    top_p, temp = 0.6, 0.8
    p = torch.softmax(logits.float() / temp, dim=-1)
    nucleus = []
    for row in p:  # shortest prefix, by decreasing probability, whose mass reaches top_p
        order = torch.argsort(row, descending=True, stable=True).tolist()
        acc, keep = 0.0, set()
        for t in order:
            keep.add(t)
            acc += row[t].item()
            if acc >= top_p:
                break
        nucleus.append(keep)
    kept = torch.isfinite(inf.filter_logits(logits, temp, 0, top_p))
    for b in range(4):
        assert set(torch.nonzero(kept[b]).flatten().tolist()) == nucleus[b]
    gen = torch.Generator().manual_seed(0)
    for _ in range(200):
        tok = inf.sample_token(logits, temp, 0, top_p, gen)
        assert all(tok[b].item() in nucleus[b] for b in range(4))
    kk = torch.isfinite(inf.filter_logits(logits, 1.0, 5, 1.0))
    assert kk.sum(-1).tolist() == [5] * 4


def test_eos_stops_that_sequence_only():
    m = _model("llama-micro")
    prompts = [[3, 4, 5], [9, 8]]
    base, _ = inf.generate(m, prompts, 20)
    eos = base[0][4]  # sequence 0 emits it as its 5th token
    cut = base[0].index(eos) + 1
    toks, why = inf.generate(m, prompts, 20, eos_id=eos)
    assert toks[0] == base[0][:cut] and why[0] == "eos"
    if eos in base[1]:
        assert toks[1] == base[1][:base[1].index(eos) + 1] and why[1] == "eos"
    else:
        assert toks[1] == base[1] and why[1] == "max_new_tokens"


def test_full_cache_ends_with_length():
    m = _model("llama-micro", seq_len=12)
    toks, why = inf.generate(m, [[1, 2, 3, 4, 5, 6, 7, 8], [1, 2]], 10)
    # 8 prompt tokens + 4 generated fill seq_len = 12 (the 5th, sampled from the last row, has no row)
    assert why == ["length", "max_new_tokens"]
    assert len(toks[0]) == 12 - 8 + 1 and len(toks[1]) == 10
    naive, why2 = inf.generate(m, [[1, 2, 3, 4, 5, 6, 7, 8], [1, 2]], 10, use_cache=False)
    assert naive == toks and why2 == why


# ---------------------------------------------------------------------------------------
def _trained(tmp_path, distributed):
    from pyrecover_amd.ckpt.sharded import save_ckpt_distributed
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
    if distributed:
        save_ckpt_distributed(m, opt, sched, None, 2, 1, str(exp / "ckpt_2"), max_keep=0)
    else:
        save_ckpt_vanilla(m, opt, sched, None, 2, 1, str(exp / "ckpt_2.pt"), max_keep=0, verify=True)
    from pyrecover_amd.ckpt import core

    core.wait_all()
    return m


@pytest.mark.parametrize("distributed", [False, True])
def test_load_model_only_bit_equal_without_optimizer_state(tmp_path, monkeypatch, distributed):
    from pyrecover_amd import _ext

    if not _ext.available():
        pytest.skip("native extension not built (the checkpoint writer is native)")
    from pyrecover_amd.ckpt import model_only, sharded

    m = _trained(tmp_path, distributed)
    read = []
    if distributed:
        real, real_state = sharded._tensor_from_manifest, sharded.read_sharded_state

        def spy(path, ent):
            read.append(ent)
            return real(path, ent)

        def spy_state(path, skip=()):
            read.append(("skip", frozenset(skip)))
            return real_state(path, skip)

        monkeypatch.setattr(sharded, "_tensor_from_manifest", spy)
        monkeypatch.setattr(sharded, "read_sharded_state", spy_state)
    else:
        real_load = torch.load

        def spy_load(*a, **kw):
            read.append(kw)
            return real_load(*a, **kw)

        monkeypatch.setattr(model_only.torch, "load", spy_load)
    torch.manual_seed(9)
    m2 = Transformer(get_preset("llama-micro", seq_len=32))
    step = model_only.load_model_only(m2, str(tmp_path), "latest", distributed=distributed, verify=not distributed)
    assert step == 2
    for (k, a), (k2, b) in zip(m.state_dict().items(), m2.state_dict().items()):
        assert k == k2 and torch.equal(a, b), k
    if distributed:
        skips = [r[1] for r in read if isinstance(r, tuple) and r[0] == "skip"]
        assert len(skips) == 1
        md = sharded.read_metadata(str(tmp_path / "exp" / "ckpt_2"))
        moments = {i.fqn for i in md.storage_data if i.fqn.startswith("optimizer.state")}
        assert moments and moments <= skips[0]  # every moment entry is skipped, i.e. never opened
        n_model = sum(1 for i in md.storage_data if i.fqn.startswith("model."))
        tensors = [r for r in read if isinstance(r, dict)]
        assert len(tensors) == n_model  # exactly the model entries were read from the shard files
    else:
        assert read and all(kw.get("mmap") is True for kw in read)  # lazily mapped: moment pages never read


def test_generate_cli_end_to_end(tmp_path):
    from pyrecover_amd import _ext

    if not _ext.available():
        pytest.skip("native extension not built (the checkpoint writer is native)")
    from pyrecover_amd.ckpt.model_only import load_model_only

    _trained(tmp_path, False)
    common = [sys.executable, os.path.join(ROOT, "generate.py"), "--checkpoint-dir", str(tmp_path), "--model-preset",
              "llama-micro", "--sequence-length", "32", "--model-dtype", "fp64", "--prompt-tokens", "3,4,5",
              "--prompt-tokens", "9,8,7,6,5", "--max-new-tokens", "12"]
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    outs = []
    for extra, name in (([], "a.jsonl"), (["--no-kv-cache"], "b.jsonl")):
        out = tmp_path / name
        r = subprocess.run(common + extra + ["--output-jsonl", str(out)], capture_output=True, text=True, env=env,
                           timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        recs = [json.loads(line) for line in out.read_text().splitlines()]
        assert len(recs) == 2
        for rec, p in zip(recs, ([3, 4, 5], [9, 8, 7, 6, 5])):
            assert rec["prompt_ids"] == p and len(rec["generated_ids"]) == 12
            assert rec["finish_reason"] == "max_new_tokens" and rec["text"] is None
            assert rec["prefill_ms"] >= 0 and rec["decode_ms_per_token"] >= 0
        outs.append([rec["generated_ids"] for rec in recs])
    assert outs[0] == outs[1]
    m = Transformer(get_preset("llama-micro", seq_len=32)).double().eval()
    load_model_only(m, str(tmp_path))
    want, _ = inf.generate(m, [[3, 4, 5], [9, 8, 7, 6, 5]], 12)
    assert outs[0] == want


def test_byte_tokenizer_decode_round_trip():
    tok = ByteTokenizer()
    for s in ("", "hello", "naïve café — 日本語 🙂", "a\nb\tc"):
        assert tok.decode(tok.encode(s)) == s
    assert tok.decode([0, 1, 2, 300, -4, 104 + 3, 105 + 3]) == "hi"
