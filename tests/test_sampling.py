"""The stateless sampling rule on the CPU: the Philox uniform, ``sample_philox_ref`` against the fp64 oracle
and its acceptance check (tests/sampling_oracles.py), greedy and non-finite rows, ``generate(sampler=
"philox")`` on a llama-micro model, the generate.py flags, and the refusal of ``graph=True`` off the GPU."""
import json
import math
import os

import pytest
import torch

from pyrecover_amd import inference as inf
from pyrecover_amd.config import get_preset
from pyrecover_amd.models.llama import Transformer
from pyrecover_amd.ops import reference as ref
from pyrecover_amd.optim import sr

from tests import sampling_oracles as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = (torch.bfloat16, torch.float16)

# Philox4x32-10 at counters {row, pos, 0, 3}: literals from the plain-integer implementation, which the
# first test pins to the Random123 known answers
STREAM3 = [
    ((0, 0, 0, 3), (0, 0), "4d7b25fc d75ee2f1 26bc1f97 c64d811c"),
    ((2, 17, 0, 3), (1234, 0), "04253a71 15e5343f 48282425 e12249b2"),
    ((15, 8191, 0, 3), (0xDEADBEEF, 0x12345678), "840a1000 d422876e 5cc4f8ad 62c3c0ad"),
]


def _hex(words):
    return " ".join(f"{int(w):08x}" for w in words)


def test_integer_philox_matches_random123_known_answers():
    assert _hex(O.philox4x32_10_int((0, 0, 0, 0), (0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert _hex(O.philox4x32_10_int((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2)) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert _hex(O.philox4x32_10_int((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344),
                                    (0xA4093822, 0x299F31D0))) == "d16cfe09 94fdcceb 5001e420 24126ea1"


@pytest.mark.parametrize("counter,key,want", STREAM3)
def test_philox_stream3_known_answers_and_u_formula(counter, key, want):
    assert _hex(O.philox4x32_10_int(counter, key)) == want
    assert _hex(sr.philox4x32_10(counter, key)) == want
    row, pos = counter[0], counter[1]
    seed = key[0] | (key[1] << 32)
    u = ref.sample_uniform(torch.full((row + 1,), pos), seed)[row].item()
    assert u == (int(want.split()[0], 16) >> 8) * 2.0 ** -24
    assert 0.0 <= u < 1.0 and float(torch.tensor(u, dtype=torch.float32)) == u  # exact in fp32
    assert O.uniform([pos] * (row + 1), seed)[row].item() == u


def test_uniform_is_a_function_of_seed_row_and_position_only():
    pos = torch.tensor([5, 6, 7, 5])
    a = ref.sample_uniform(pos, 11)
    assert torch.equal(a, O.uniform(pos, 11))
    assert a[0] != a[3]  # same position, another row
    assert torch.equal(ref.sample_uniform(pos[:2], 11), a[:2])  # not of the batch size
    assert not torch.equal(ref.sample_uniform(pos, 12), a)
    assert torch.equal(ref.sample_uniform(pos, 11 + (1 << 64)), a)  # the seed is taken mod 2^64
    assert not torch.equal(ref.sample_uniform(pos, 11 + (1 << 32)), a)  # and its high word is key word 1


# ---------------------------------------------------------------------------------------
def _case_seed(dtype, V, kind):
    return 1000 * DTYPES.index(dtype) + 10 * O.VOCABS.index(V) + O.KINDS.index(kind)


@pytest.mark.parametrize("V", O.VOCABS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_reference_is_accepted_on_the_grid(dtype, V):
    bad = []
    for kind in O.KINDS:
        x = O.make_logits(kind, 3, V, dtype, _case_seed(dtype, V, kind))
        rk = O.Ranking(x)
        for n, (T, k, p) in enumerate(O.SETTINGS):
            pos = torch.tensor([n, 100 + n, 8000 + n])
            tok = ref.sample_philox_ref(x, pos, T, k, p, seed=7)
            ok = rk.accepted(tok, O.uniform(pos, 7), T, k, p)
            bad += [(kind, T, k, p, b) for b in range(3) if not ok[b]]
    assert not bad, bad


def test_every_seeded_defect_is_rejected():
    """The check would be worthless if it accepted a sampler that ignores the temperature, top-k or top-p,
    mirrors u, or is off by one in k."""
    rejected = {d: 0 for d in O.DEFECTS}
    total = 0
    for dtype in DTYPES:
        for V in (257, 2051):
            for kind in ("normal", "peaked", "ties"):
                x = O.make_logits(kind, 3, V, dtype, _case_seed(dtype, V, kind))
                rk = O.Ranking(x)
                for n, (T, k, p) in enumerate(O.SETTINGS):
                    u = O.uniform(torch.tensor([n, 100 + n, 8000 + n]), 7)
                    assert rk.accepted(rk.token(u, T, k, p), u, T, k, p).all()
                    total += 3
                    for d in O.DEFECTS:
                        rejected[d] += int((~rk.accepted(O.defect_token(d, rk, u, T, k, p), u, T, k, p)).sum())
    assert all(n >= 1 for n in rejected.values()), (rejected, total)


def test_greedy_equals_greedy_token_with_ties_and_minus_inf():
    g = torch.Generator().manual_seed(3)
    for dtype in DTYPES + (torch.float32,):
        x = torch.randn(6, 300, generator=g).to(dtype)
        x[1, [250, 17, 99]] = x[1].max() + 1  # ties: the lowest id wins
        x[2] = 0.25
        x[3, 5:] = float("-inf")
        x[4] = float("-inf")
        x[5, 7], x[5, 9] = -0.0, 0.0  # one value
        x[5, :7], x[5, 8], x[5, 10:] = -1.0, -1.0, -1.0
        want = inf.greedy_token(x)
        assert want.tolist()[1:] == [17, 0, x[3, :5].argmax().item(), 0, 7]
        assert torch.equal(ref.sample_philox_ref(x, torch.zeros(6), 0.0), want)
        assert torch.equal(ref.greedy_total_order(x), want)
        assert torch.equal(O.Ranking(x).token(torch.zeros(6), 0.0), want)
        assert torch.equal(inf.sample_philox(x, torch.zeros(6, dtype=torch.long), 0.0), want)


@pytest.mark.parametrize("dtype", DTYPES + (torch.float32,), ids=["bf16", "fp16", "fp32"])
def test_nonfinite_rows_follow_the_total_order(dtype):
    x, want = O.nonfinite_rows(dtype)
    pos = torch.arange(6)
    for T, k, p in ((0.0, 0, 1.0), (1.0, 0, 1.0), (0.7, 5, 0.9)):
        tok = ref.sample_philox_ref(x, pos, T, k, p, seed=1)
        assert tok.tolist() == want, (T, k, p)  # row 1: a 28-nat lead over the rest, every u picks it
        assert O.Ranking(x).accepted(tok, O.uniform(pos, 1), T, k, p).all()


def test_top_k_one_with_a_unique_maximum_is_greedy_for_every_u():
    x = O.make_logits("peaked", 64, 500, torch.bfloat16, 5)
    want = inf.greedy_token(x)
    for seed in range(4):
        tok = ref.sample_philox_ref(x, torch.arange(64) * 3, 1.3, 1, 1.0, seed)
        assert torch.equal(tok, want)


def test_frequencies_follow_the_distribution():
    """4096 rows of one 8-token distribution, pos = arange: the rows whose u lies within DELTA of a
    boundary are at most 1% (a property of the seed), every other row equals the oracle's token, and the
    per-token counts lie within 5 binomial sigma."""
    tok, rk, u = O.frequency_case(lambda x, pos, seed: ref.sample_philox_ref(x, pos, 1.0, 0, 1.0, seed))
    O.check_frequencies(tok, rk, u)


# ---------------------------------------------------------------------------------------
def _model(seq_len=64, seed=0, dtype=torch.float64):
    torch.manual_seed(seed)
    return Transformer(get_preset("llama-micro", seq_len=seq_len)).to(dtype).eval()


def test_generate_philox_is_seeded_and_position_indexed():
    m = _model()
    prompts = [[3, 4, 5, 6, 7], [9, 8]]  # ragged
    kw = dict(temperature=0.9, top_k=40, top_p=0.95, sampler="philox")
    a, why = inf.generate(m, prompts, 24, seed=5, **kw)
    b, _ = inf.generate(m, prompts, 24, seed=5, **kw)
    c, _ = inf.generate(m, prompts, 24, seed=6, **kw)
    assert a == b and a != c and why == ["max_new_tokens"] * 2
    naive, why2 = inf.generate(m, prompts, 24, seed=5, use_cache=False, **kw)
    assert naive == a and why2 == why  # draws are indexed by position, not by step
    # the draw of row 0 at position 5 + i is a function of (seed, row, position) and the logits alone:
    # generating 10 tokens gives the first 10 of the 24
    short, _ = inf.generate(m, prompts, 10, seed=5, **kw)
    assert short == [t[:10] for t in a]
    # and the default sampler is untouched by the new argument
    t0, _ = inf.generate(m, prompts, 8, temperature=0.8, seed=3)
    t1, _ = inf.generate(m, prompts, 8, temperature=0.8, seed=3, sampler="torch")
    assert t0 == t1
    # temperature 0: both samplers are greedy
    g0, _ = inf.generate(m, prompts, 8)
    g1, _ = inf.generate(m, prompts, 8, sampler="philox")
    assert g0 == g1


def test_generate_philox_eos_and_length():
    m = _model()
    prompts = [[3, 4, 5], [9, 8]]
    kw = dict(temperature=0.8, seed=2, sampler="philox")
    base, _ = inf.generate(m, prompts, 20, **kw)
    eos = base[0][4]
    cut = base[0].index(eos) + 1
    toks, why = inf.generate(m, prompts, 20, eos_id=eos, **kw)
    assert toks[0] == base[0][:cut] and why[0] == "eos"
    if eos in base[1]:
        assert toks[1] == base[1][:base[1].index(eos) + 1] and why[1] == "eos"
    else:
        assert toks[1] == base[1] and why[1] == "max_new_tokens"
    m12 = _model(seq_len=12)
    toks, why = inf.generate(m12, [[1, 2, 3, 4, 5, 6, 7, 8], [1, 2]], 10, **kw)
    assert why == ["length", "max_new_tokens"] and [len(t) for t in toks] == [12 - 8 + 1, 10]
    naive, why2 = inf.generate(m12, [[1, 2, 3, 4, 5, 6, 7, 8], [1, 2]], 10, use_cache=False, **kw)
    assert naive == toks and why2 == why


def test_generate_rejects_an_unknown_sampler_and_a_graph_on_the_cpu():
    m = _model()
    with pytest.raises(ValueError, match="sampler"):
        inf.generate(m, [[1, 2]], 4, sampler="gumbel")
    with pytest.raises(ValueError, match="sampler='philox' or temperature 0"):
        inf.generate(m, [[1, 2]], 4, temperature=0.7, graph=True)
    with pytest.raises(ValueError, match="use_cache=False"):
        inf.generate(m, [[1, 2]], 4, sampler="philox", graph=True, use_cache=False)
    with pytest.raises(ValueError, match="bf16 / fp16 model on the GPU"):
        inf.generate(m.cpu(), [[1, 2]], 4, temperature=0.7, sampler="philox", graph=True)
    with pytest.raises(ValueError, match="bf16 / fp16 model on the GPU"):
        inf.generate(m.cpu(), [[1, 2]], 4, graph=True)  # greedy: still no GPU model


def test_cli_flags_and_jsonl_fields(tmp_path, monkeypatch):
    from pyrecover_amd import _ext, generate as gen_cli

    a = gen_cli.build_parser().parse_args(["--prompt-tokens", "1,2"])
    assert a.sampler == "torch" and a.decode_graph is False  # defaults unchanged
    a = gen_cli.build_parser().parse_args(["--prompt-tokens", "1,2", "--sampler", "philox", "--decode-graph"])
    assert a.sampler == "philox" and a.decode_graph is True
    with pytest.raises(SystemExit):
        gen_cli.build_parser().parse_args(["--prompt-tokens", "1,2", "--sampler", "gumbel"])
    if not _ext.available():
        pytest.skip("native extension not built (the checkpoint writer is native)")
    from pyrecover_amd.ckpt import core
    from pyrecover_amd.ckpt.vanilla import save_ckpt_vanilla
    from pyrecover_amd.optim.adamw import FlatAdamW
    from pyrecover_amd.optim.lr import build_lr_scheduler

    torch.manual_seed(0)
    m = Transformer(get_preset("llama-micro", seq_len=32))
    opt = FlatAdamW(m.flatten_(), lr=1e-2)
    exp = tmp_path / "exp"
    exp.mkdir()
    save_ckpt_vanilla(m, opt, build_lr_scheduler(opt, 2), None, 1, 1, str(exp / "ckpt_1.pt"), max_keep=0, verify=True)
    core.wait_all()
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)  # generate.py picks the device from this
    out = tmp_path / "o.jsonl"
    argv = ["--checkpoint-dir", str(tmp_path), "--model-preset", "llama-micro", "--sequence-length", "32",
            "--model-dtype", "fp64", "--prompt-tokens", "3,4,5", "--max-new-tokens", "6", "--temperature", "0.8",
            "--seed", "4", "--sampler", "philox", "--output-jsonl", str(out)]
    assert gen_cli.main(argv) == 0
    rec = json.loads(out.read_text().splitlines()[0])
    assert rec["sampler"] == "philox" and rec["decode_graph"] is False and len(rec["generated_ids"]) == 6
    want, _ = inf.generate(m.double().eval(), [[3, 4, 5]], 6, temperature=0.8, seed=4, sampler="philox")
    assert rec["generated_ids"] == want[0]
    with pytest.raises(ValueError, match="graph=True refused"):
        gen_cli.main(argv + ["--decode-graph"])
    assert math.isfinite(rec["decode_ms_per_token"])
