"""hipGraph-captured decode (inference.DecodeGraph, generate(graph=True)) against the eager paths:
greedy tokens equal today's eager output, philox tokens equal eager philox token for token, eos and a
full cache end rows as eager does, the graph's logits are the eager decode_step's bits, and generate.py
--sampler philox --decode-graph runs from a train.py checkpoint."""
import json
import os
import subprocess
import sys

import pytest
import torch

from pyrecover_amd import inference as inf
from pyrecover_amd.config import get_preset
from pyrecover_amd.models.llama import Transformer

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROMPTS = [[3, 4, 5, 6, 7, 8, 9], [9, 8], [1, 2, 3, 4]]  # ragged
# llama-micro is GQA 2:1 at head_dim 64; n_kv_heads = 2 makes it MHA
MODELS = [(torch.bfloat16, {}), (torch.float16, {"n_kv_heads": 2}), (torch.bfloat16, {"n_kv_heads": 2}),
          (torch.float16, {})]
IDS = ["bf16-gqa", "fp16-mha", "bf16-mha", "fp16-gqa"]


def _model(cuda, dtype, over, seq_len=96):
    torch.manual_seed(0)
    return Transformer(get_preset("llama-micro", seq_len=seq_len, **over)).to(cuda).to(dtype).eval()


@pytest.mark.parametrize("dtype,over", MODELS, ids=IDS)
def test_greedy_graph_equals_todays_eager_output(cuda, dtype, over):
    m = _model(cuda, dtype, over)
    want, why = inf.generate(m, PROMPTS, 40)  # sampler="torch", eager
    stats = {}
    got, why_g = inf.generate(m, PROMPTS, 40, graph=True, stats=stats)
    assert got == want and why_g == why == ["max_new_tokens"] * 3
    assert stats["graph_replays"] == 40 - 1 - inf.DecodeGraph.WARMUP and stats["decode_steps"] == 39
    eager_dev, _ = inf.generate(m, PROMPTS, 40, sampler="philox")  # the kernel's greedy, no graph
    assert eager_dev == want


@pytest.mark.parametrize("dtype,over", MODELS, ids=IDS)
def test_sampled_graph_equals_eager_philox(cuda, dtype, over):
    m = _model(cuda, dtype, over)
    kw = dict(temperature=0.9, top_k=50, top_p=0.95, seed=13, sampler="philox")
    n = 2 * inf.SYNC_EVERY + 12  # crosses the read-back of the finished mask twice
    want, why = inf.generate(m, PROMPTS, n, **kw)
    got, why_g = inf.generate(m, PROMPTS, n, graph=True, **kw)
    assert got == want and why_g == why
    again, _ = inf.generate(m, PROMPTS, n, graph=True, **kw)
    assert again == got
    other, _ = inf.generate(m, PROMPTS, n, graph=True, **dict(kw, seed=14))
    assert other != got
    assert len({tuple(t) for t in got}) == 3 and all(len(set(t)) > 4 for t in got)  # draws, not a constant


def test_eos_and_full_cache_end_rows_as_eager(cuda):
    m = _model(cuda, torch.bfloat16, {})
    kw = dict(temperature=0.8, seed=2, sampler="philox")
    base, _ = inf.generate(m, PROMPTS, 40, **kw)
    eos = base[0][20]  # row 0 emits it mid-run (at its first occurrence, token 20 at the latest)
    want, why = inf.generate(m, PROMPTS, 40, eos_id=eos, **kw)
    got, why_g = inf.generate(m, PROMPTS, 40, eos_id=eos, graph=True, **kw)
    assert got == want and why_g == why and why[0] == "eos"
    assert want[0] == base[0][:base[0].index(eos) + 1]
    for b in (1, 2):
        cut = base[b].index(eos) + 1 if eos in base[b] else 40
        assert want[b] == base[b][:cut]
    # greedy with eos, against the torch-sampler eager path
    g_base, _ = inf.generate(m, PROMPTS, 40)
    g_eos = g_base[1][10]
    assert inf.generate(m, PROMPTS, 40, eos_id=g_eos, graph=True) == inf.generate(m, PROMPTS, 40, eos_id=g_eos)
    # every row done before max_new_tokens: the loop leaves at a read-back and the outputs still agree
    stats = {}
    a = inf.generate(m, [[5, 6]], 60, eos_id=g_eos, graph=True, stats=stats)
    assert a == inf.generate(m, [[5, 6]], 60, eos_id=g_eos)
    # cache full: 20 rows, prompts of 12 and 2 tokens, 30 wanted
    m20 = _model(cuda, torch.bfloat16, {}, seq_len=20)
    long_p = [list(range(1, 13)), [1, 2]]
    for extra in (dict(), kw):
        want, why = inf.generate(m20, long_p, 30, **extra)
        got, why_g = inf.generate(m20, long_p, 30, graph=True, **extra)
        assert got == want and why_g == why == ["length", "length"]
        assert [len(t) for t in got] == [20 - 12 + 1, 20 - 2 + 1]


@pytest.mark.parametrize("dtype,over", MODELS[:2], ids=IDS[:2])
def test_graph_logits_are_the_eager_decode_step_bits(cuda, dtype, over):
    m = _model(cuda, dtype, over)
    cfg = m.model_args
    B, N = 3, 9
    lens = torch.tensor([len(p) for p in PROMPTS], device=cuda)
    buf = torch.zeros(B, 7, dtype=torch.long, device=cuda)
    for b, p in enumerate(PROMPTS):
        buf[b, :len(p)] = torch.tensor(p)
    runs = []
    for use_graph in (False, True):
        cache = inf.KVCache(cfg, B, 48, dtype, cuda)
        logits = inf.prefill(m, buf, lens, cache)
        ds = inf.DeviceSampler(lens, 48 - lens, 32, temperature=1.1, top_k=0, top_p=0.9, seed=4)
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
                     cache._v.clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert runs[0][2].tolist() == [N] * B and runs[0][3].tolist() == (lens + N).tolist()


def test_graph_is_refused_with_its_reason(cuda):
    m = _model(cuda, torch.bfloat16, {})
    with pytest.raises(ValueError, match="sampler='philox' or temperature 0"):
        inf.generate(m, PROMPTS, 4, temperature=0.7, graph=True)
    with pytest.raises(ValueError, match="use_cache=False"):
        inf.generate(m, PROMPTS, 4, graph=True, use_cache=False)
    with pytest.raises(ValueError, match="bf16 / fp16 model on the GPU"):
        inf.generate(m.float(), PROMPTS, 4, graph=True)


def test_generate_py_decode_graph_from_a_train_py_checkpoint(cuda, tmp_path):
    train = [sys.executable, os.path.join(ROOT, "train.py"), "--model-preset", "llama-micro", "--synthetic-data",
             "--batch-size", "2", "--sequence-length", "128", "--training-steps", "2", "--checkpoint-frequency", "2",
             "--logging-frequency", "1", "--num-workers", "0", "--checkpoint-dir", str(tmp_path),
             "--experiment_name", "gen"]
    r = subprocess.run(train, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    gen = [sys.executable, os.path.join(ROOT, "generate.py"), "--model-preset", "llama-micro", "--sequence-length",
           "128", "--checkpoint-dir", str(tmp_path), "--prompt-tokens", "3,4,5", "--prompt-tokens", "9,8,7,6,5,4,3",
           "--max-new-tokens", "24", "--temperature", "0.8", "--top-k", "50", "--top-p", "0.95", "--seed", "11",
           "--sampler", "philox"]
    outs = []
    for extra, name in ((["--decode-graph"], "a.jsonl"), ([], "b.jsonl")):
        out = tmp_path / name
        r = subprocess.run(gen + extra + ["--output-jsonl", str(out)], capture_output=True, text=True, timeout=300,
                           cwd=ROOT)
        assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
        assert "runs PyTorch math" not in r.stderr
        recs = [json.loads(line) for line in out.read_text().splitlines()]
        assert [len(x["generated_ids"]) for x in recs] == [24, 24]
        assert all(x["sampler"] == "philox" and x["decode_graph"] is bool(extra) for x in recs)
        assert all(x["finish_reason"] == "max_new_tokens" and x["decode_ms_per_token"] > 0 for x in recs)
        outs.append([x["generated_ids"] for x in recs])
    assert outs[0] == outs[1]
