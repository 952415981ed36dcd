"""extend on an fp8 KV cache on the CPU (torch-math path): one extend against T decode steps in fp64, the
fp8_extend flag, and the multi-token rope_append_fp8_ref against kv_quantize_ref of what rope_append_ref writes."""
import pytest
import torch

from pyrecover_amd import inference as inf
from pyrecover_amd.ops import reference as ref
from tests.test_extend import TOL, _model, _ragged


def test_extend_fp8_equals_decode_steps():
    """fp64 llama-micro, fp8 caches: one 5-token extend with fp8_extend=True against 5 decode steps. Quantization is
    discontinuous: keys equal to 1e-16 could round to different bytes. At this seed they do not, which is checked here."""
    m = _model("llama-micro")
    _, prompt, app = _ragged(m, [3, 8], [5, 5], seed=3)
    a, b = (inf.KVCache(m.model_args, 2, 16, torch.float64, "cpu", kv_dtype="fp8") for _ in range(2))
    for c in (a, b):
        inf.prefill(m, prompt, torch.tensor([3, 8]), c)
    steps = torch.stack([inf.decode_step(m, app[:, t], a) for t in range(5)], 1)
    rows = inf.extend(m, app, torch.tensor([5, 5]), b, return_all=True, fp8_extend=True)
    assert a.kv_len.tolist() == b.kv_len.tolist() == [8, 13]
    assert all(torch.equal(x, y) for x, y in zip(a.k + a.v + a.k_scale + a.v_scale, b.k + b.v + b.k_scale + b.v_scale))
    assert (steps - rows).abs().max().item() < TOL


def test_fp8_extend_flag_gates_fp8_only():
    m = _model("llama-micro", dtype=torch.float32)
    tok, n = torch.tensor([[3, 4, 5], [9, 8, 7]]), torch.tensor([3, 3])
    cache = inf.KVCache(m.model_args, 2, 16, torch.float32, "cpu", kv_dtype="fp8")
    with pytest.raises(ValueError, match="fp8_extend=True"):
        inf.extend(m, tok, n, cache)
    assert torch.isfinite(inf.prefill(m, tok, n, cache, chunk=2, fp8_extend=True)).all()
    assert torch.isfinite(inf.extend(m, tok, n, cache, fp8_extend=True)).all() and cache.kv_len.tolist() == [6, 6]
    assert inf.generate(m, [[3, 4, 5]], 4, kv_cache_dtype="fp8", prefill_chunk=2, fp8_extend=True)[1] == ["max_new_tokens"]
    got = []
    for flag in (False, True):  # a cache in the model's dtype: the flag changes nothing
        c = inf.KVCache(m.model_args, 2, 16, torch.float32, "cpu")
        got.append((inf.prefill(m, tok, n, c, chunk=2, fp8_extend=flag), inf.extend(m, tok, n, c, fp8_extend=flag),
                    inf.generate(m, [[3, 4, 5]], 4, prefill_chunk=2, fp8_extend=flag)))
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1]) and got[0][2] == got[1][2]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_rope_append_fp8_ref_multi_token_bits(dtype):
    """T = 5 at bases 0, 7, cap - 2 (three tokens overflow and store nothing) and beyond the capacity."""
    B, T, cap, Hq, Hkv, D = 4, 5, 12, 4, 2, 16
    torch.manual_seed(0)
    tab = ref.rope_table(ref.precompute_freqs_cis(D, cap))
    q16 = (torch.randn(B * T, (Hq + 2 * Hkv) * D) * 3).to(dtype)
    n, q8 = torch.tensor([0, 7, cap - 2, cap + 4]), q16.clone()
    kc, vc = (torch.full((B, cap, Hkv, D), 5.0, dtype=dtype) for _ in range(2))
    ref.rope_append_ref(q16, tab, n, kc, vc)
    kq, vq = (torch.full((B, cap, Hkv, D), 0xAB, dtype=torch.uint8) for _ in range(2))
    ks, vs = (torch.full((B, cap, Hkv), 7.0) for _ in range(2))
    ref.rope_append_fp8_ref(q8, tab, n, kq, vq, ks, vs)
    written = ((pos := torch.arange(cap).view(1, cap)) >= n.view(B, 1)) & (pos < (n + T).view(B, 1))
    assert torch.equal(q8, q16) and written.sum().item() == 5 + 5 + 2
    for c16, cq, cs in ((kc, kq, ks), (vc, vq, vs)):
        wq, ws = ref.kv_quantize_ref(c16)
        assert torch.equal(cq[written], wq[written]) and torch.equal(cs[written], ws[written])
        assert bool((cq[~written] == 0xAB).all()) and bool((cs[~written] == 7.0).all())
