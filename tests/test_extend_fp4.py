"""extend on an MXFP4 KV cache on the CPU (torch-math path): one extend against T decode steps in fp64, the chunked
prefill against the matching extends, and the fp4_extend flag through extend / prefill / generate / the CLI."""
import pytest
import torch

from pyrecover_amd import inference as inf
from pyrecover_amd.generate import build_parser
from tests.test_extend import TOL, _model, _ragged


def _bytes(c):
    return c.k + c.v + c.k_scale + c.v_scale


def test_extend_fp4_equals_decode_steps():
    """fp64 llama-micro, fp4 caches: one 5-token extend with fp4_extend=True against 5 decode steps: equal cache
    bytes (a key within 1e-16 of a rounding boundary could differ; at this seed none does), logits within TOL."""
    m = _model("llama-micro")
    _, prompt, app = _ragged(m, [3, 8], [5, 5], seed=3)
    a, b = (inf.KVCache(m.model_args, 2, 16, torch.float64, "cpu", kv_dtype="fp4") for _ in range(2))
    for c in (a, b):
        inf.prefill(m, prompt, torch.tensor([3, 8]), c)
    steps = torch.stack([inf.decode_step(m, app[:, t], a) for t in range(5)], 1)
    rows = inf.extend(m, app, torch.tensor([5, 5]), b, return_all=True, fp4_extend=True)
    assert a.kv_len.tolist() == b.kv_len.tolist() == [8, 13]
    assert all(torch.equal(x, y) for x, y in zip(_bytes(a), _bytes(b)))
    assert (steps - rows).abs().max().item() < TOL


def test_chunked_prefill_fp4_is_successive_extends():
    m = _model("llama-micro")
    tok, lens = torch.randint(0, m.model_args.vocab_size, (2, 5), generator=torch.Generator().manual_seed(1)), torch.tensor([5, 4])
    a, b = (inf.KVCache(m.model_args, 2, 8, torch.float64, "cpu", kv_dtype="fp4") for _ in range(2))
    logits = inf.prefill(m, tok, lens, a, chunk=2, fp4_extend=True)
    for c0 in (0, 2, 4):
        piece = tok[:, c0:c0 + 2]
        last = inf.extend(m, piece, torch.full((2,), piece.shape[1]), b, return_all=True, fp4_extend=True)
    assert a.kv_len.tolist() == [5, 4] and b.kv_len.tolist() == [5, 5]
    assert all(torch.equal(x[:, :5], y[:, :5]) for x, y in zip(_bytes(a), _bytes(b)))
    assert torch.equal(logits[0], last[0, 0])  # row 4 lies in the last piece


def test_fp4_extend_flag_gates_fp4_only():
    m = _model("llama-micro", dtype=torch.float32)
    tok, n = torch.tensor([[3, 4, 5], [9, 8, 7]]), torch.tensor([3, 3])
    cache = inf.KVCache(m.model_args, 2, 16, torch.float32, "cpu", kv_dtype="fp4")
    for call in (lambda **kw: inf.extend(m, tok, n, cache, **kw), lambda **kw: inf.prefill(m, tok, n, cache, chunk=2, **kw),
                 lambda **kw: inf.generate(m, [[3, 4, 5]], 4, kv_cache_dtype="fp4", prefill_chunk=2, **kw)):
        for kw in ({}, {"fp8_extend": True}):
            with pytest.raises(ValueError, match="fp4_extend=True"):
                call(**kw)
    assert torch.isfinite(inf.prefill(m, tok, n, cache, chunk=2, fp4_extend=True)).all()
    assert torch.isfinite(inf.extend(m, tok, n, cache, fp4_extend=True)).all() and cache.kv_len.tolist() == [6, 6]
    kw = dict(kv_cache_dtype="fp4", fp4_extend=True)
    assert inf.generate(m, [[3, 4, 5]], 4, prefill_chunk=2, **kw)[1] == ["max_new_tokens"]
    # the one-shot prefill is untouched by the flag: the first token is the 16-bit cache's
    assert inf.generate(m, [[3, 4, 5]], 1, **kw)[0] == inf.generate(m, [[3, 4, 5]], 1)[0]
    c8 = inf.KVCache(m.model_args, 2, 16, torch.float32, "cpu", kv_dtype="fp8")
    with pytest.raises(ValueError, match="fp8_extend=True"):  # the fp4 flag does not open an fp8 cache
        inf.extend(m, tok, n, c8, fp4_extend=True)
    c16 = [inf.KVCache(m.model_args, 2, 16, torch.float32, "cpu") for _ in range(2)]  # there the flag changes nothing
    got = [(inf.prefill(m, tok, n, c, chunk=2, fp4_extend=f), inf.extend(m, tok, n, c, fp4_extend=f)) for c, f in zip(c16, (False, True))]
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])
    args = build_parser().parse_args(["--kv-cache-dtype", "fp4", "--prefill-chunk", "512", "--fp4-extend"])
    assert args.fp4_extend and not build_parser().parse_args([]).fp4_extend
