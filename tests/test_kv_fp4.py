"""MXFP4 KV cache on the CPU: ops/reference.py's rule against the table oracle of tests/kv_fp4_oracles.py,
KVCache(kv_dtype="fp4") through prefill / decode_step / generate, and the refusals."""
import pytest
import torch

from pyrecover_amd import inference as inf
from pyrecover_amd.config import get_preset
from pyrecover_amd.models.llama import Transformer
from pyrecover_amd.ops import reference as ref
from tests import attention_oracles as A
from tests import kv_fp4_oracles as Q
from tests.kv_fp8_oracles import random_rows

DTYPES = (torch.bfloat16, torch.float16)


@pytest.mark.parametrize("dtype", DTYPES, ids=A.dname)
@pytest.mark.parametrize("D", [64, 128])
def test_reference_equals_the_table_oracle(D, dtype):
    """Random rows over 40 binades and the edge rows: same bits; dequantize equals the oracle's and is idempotent."""
    x = torch.cat([random_rows(dtype, 400, D), Q.edge_rows(dtype, D)])
    q, s = ref.kv_quantize_fp4_ref(x)
    wq, ws = Q.quantize(x)
    assert q.dtype == s.dtype == torch.uint8 and q.shape == (len(x), D // 2) and s.shape == (len(x), D // 32)
    assert torch.equal(q, wq) and torch.equal(s, ws)
    assert torch.equal(ref.kv_dequantize_fp4_ref(q, s, torch.float64), Q.dequantize(wq, ws))
    # exact in fp32 too, but for the last edge row: a block maximum of the largest bf16 rounds up to 4 * 2^126 = 2^128
    d = ref.kv_dequantize_fp4_ref(q[:-1], s[:-1])
    assert d.dtype == torch.float32 and torch.equal(d.double(), Q.dequantize(wq[:-1], ws[:-1]))
    q2, s2 = ref.kv_quantize_fp4_ref(d)
    assert torch.equal(ref.kv_dequantize_fp4_ref(q2, s2), d)  # idempotent (the scale of a block may shrink)


def _model(preset="llama-micro", seq_len=64, dtype=torch.float64, **kw):
    torch.manual_seed(0)
    return Transformer(get_preset(preset, seq_len=seq_len, **kw)).to(dtype).eval()


@pytest.mark.parametrize("preset", ["llama-micro", "llama-tiny"])
def test_cache_size_and_layout(preset):
    a = get_preset(preset, seq_len=64)
    c16 = inf.KVCache(a, 3, 40, torch.bfloat16, "cpu")
    c4 = inf.KVCache(a, 3, 40, torch.bfloat16, "cpu", kv_dtype="fp4")
    D = a.head_dim
    assert c4.nbytes() * 2 * D == c16.nbytes() * (D // 2 + D // 32)
    assert c4.k[0].dtype == torch.uint8 and c4.k[0].shape == (3, 40, a.kv_heads, D // 2)
    assert c4.v_scale[0].dtype == torch.uint8 and c4.v_scale[0].shape == (3, 40, a.kv_heads, D // 32)
    assert bool((c4.k_scale[0] == 127).all()) and c4.fp4 and not c4.fp8 and c4.kv_dtype == "fp4" and not c16.fp4


def test_fp64_generate_and_the_stored_cache():
    """The first token is the model cache's; the cache holds the oracle applied to what the model-dtype cache holds."""
    m = _model("llama-tiny")
    prompts = [[5, 9, 2], [7, 1, 4, 4, 8, 3, 11, 6]]
    base, _ = inf.generate(m, prompts, 8)
    got, why = inf.generate(m, prompts, 8, kv_cache_dtype="fp4")
    assert why == ["max_new_tokens"] * 2 and [t[0] for t in got] == [t[0] for t in base]
    toks = torch.randint(0, m.vocab_size, (2, 9), generator=torch.Generator().manual_seed(4))
    c, c4 = (inf.KVCache(m.model_args, 2, 16, torch.float64, "cpu", kv_dtype=k) for k in ("model", "fp4"))
    assert torch.equal(inf.prefill(m, toks, torch.tensor([9, 4]), c), inf.prefill(m, toks, torch.tensor([9, 4]), c4))
    inf.decode_step(m, toks[:, 0], c), inf.decode_step(m, toks[:, 0], c4)
    for b, n in enumerate([9, 4]):  # layer 0, whose appended row depends on no cache
        wq, ws = Q.quantize(c.k[0][b, :n + 1])
        assert torch.equal(c4.k[0][b, :n + 1], wq) and torch.equal(c4.k_scale[0][b, :n + 1], ws)


def test_refusals():
    m = _model("llama-micro")
    toks = torch.zeros(2, 4, dtype=torch.long)
    c4 = inf.KVCache(m.model_args, 2, 8, torch.float64, "cpu", kv_dtype="fp4")
    for flag in (False, True):
        with pytest.raises(ValueError, match="fp4"):
            inf.extend(m, toks, torch.tensor([4, 4]), c4, fp8_extend=flag)
        with pytest.raises(ValueError, match="fp4"):
            inf.prefill(m, toks, torch.tensor([4, 4]), c4, chunk=2, fp8_extend=flag)
        with pytest.raises(ValueError, match="fp4"):
            inf.generate(m, [[3, 4, 5]], 4, kv_cache_dtype="fp4", prefill_chunk=2, fp8_extend=flag)
    with pytest.raises(ValueError, match="paged fp4"):
        inf.PagedKVCache(m.model_args, 1, 64, torch.float64, "cpu", kv_dtype="fp4")
    with pytest.raises(ValueError, match="paged fp4"):
        inf.generate(m, [[3, 4, 5]], 4, kv_cache_dtype="fp4", kv_page_size=64)
    with pytest.raises(ValueError, match="needs the KV cache"):
        inf.generate(m, [[3, 4, 5]], 4, kv_cache_dtype="fp4", use_cache=False)
    c4.k_scale[0] = c4.k_scale[0][:, :4]
    with pytest.raises(ValueError, match="fp4 cache holds"):
        inf.prefill(m, toks, torch.tensor([4, 4]), c4)
    with pytest.raises(ValueError, match="multiple of 32"):
        inf.KVCache(get_preset("llama-micro", seq_len=64, dim=96, n_heads=2, n_kv_heads=2), 1, 8, torch.float32, "cpu",
                    kv_dtype="fp4")
