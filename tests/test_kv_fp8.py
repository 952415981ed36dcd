"""fp8 KV cache on the CPU: the format rule (ops/reference.py against the integer / fp64 oracle of
tests/kv_fp8_oracles.py), its properties, the seeded defects the comparison must catch, the plumbing of
KVCache(kv_dtype="fp8") through prefill / decode_step / generate, and the generate.py flag."""
import json
import os
import subprocess
import sys

import pytest
import torch

from pyrecover_amd import inference as inf
from pyrecover_amd.config import get_preset
from pyrecover_amd.models.llama import Transformer
from pyrecover_amd.ops import reference as ref
from tests import attention_oracles as A
from tests import kv_fp8_oracles as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = (torch.bfloat16, torch.float16)


def _rows(dtype, D=128):
    return torch.cat([Q.random_rows(dtype, 4096, D), Q.edge_rows(dtype, D)])


@pytest.mark.parametrize("dtype", DTYPES, ids=A.dname)
def test_reference_equals_oracle_and_the_rule_holds(dtype):
    x = _rows(dtype)
    q, s = ref.kv_quantize_ref(x)
    qo, so = Q.quantize(x)
    assert q.dtype == torch.uint8 and s.dtype == torch.float32 and q.shape == x.shape and s.shape == x.shape[:-1]
    assert torch.equal(q, qo) and torch.equal(s, so)
    # scales are powers of two; an all-zero row (also of -0.0) has scale 1 and bytes 0
    m, _ = torch.frexp(s)
    assert bool((m == 0.5).all())
    zero = x.float().abs().amax(-1) == 0
    assert int(zero.sum()) >= 2 and bool((s[zero] == 1).all()) and bool((q[zero] == 0).all())
    # scaled row maxima lie in (224, 448] unless e was clamped at -126
    x64 = x.double()
    amax = x64.abs().amax(-1)
    live = ~zero & (s.double() > 2.0 ** -126)
    top = amax[live] / s.double()[live]
    assert bool((top > 224).all()) and bool((top <= 448).all())
    assert bool((amax[~zero] / s.double()[~zero] <= 448).all())
    # dequantized values: the reference equals the oracle, round-trips through 16 bits, and is within amax / 16
    # (one corner is outside the round trip: a row whose amax is within 1/16 of the top of the dtype's last
    # binade rounds up to 256 * 2^e = twice that binade's base, which bf16 and fp32 (2^128) or fp16 (2^16) do
    # not hold; only the row of the dtype's largest finite value does that here)
    d = Q.dequantize(q, s)
    over = d.abs() > torch.finfo(dtype).max
    assert int(over.sum()) == 1 and bool((x.float().abs()[over] == torch.finfo(dtype).max).all())
    assert torch.equal(ref.kv_dequantize_ref(q, s).double()[d.abs() <= torch.finfo(torch.float32).max],
                       d[d.abs() <= torch.finfo(torch.float32).max])
    # byte * scale is not below the dtype's subnormal range
    fits = ((s.double() >= (2.0 ** -24 if dtype == torch.float16 else 2.0 ** -133) * 512)[:, None] & ~over)
    for t in DTYPES:
        if t == torch.float16 and dtype == torch.bfloat16:
            continue  # bf16 rows span binades fp16 does not have
        assert torch.equal(ref.kv_dequantize_ref(q, s, t).double()[fits], d[fits]), t
    err = (d - x64).abs()
    assert bool((err <= amax[:, None] / 16).all())
    print(f"max |dequant - x| / amax = {float((err / amax.clamp_min(1e-300)[:, None]).max()):.4f}")


def test_fp64_and_fp32_inputs_are_taken_as_fp32():
    x = torch.randn(64, 64, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    for t in (x, x.float()):
        q, s = ref.kv_quantize_ref(t)
        qo, so = Q.quantize(x.float())
        assert torch.equal(q, qo) and torch.equal(s, so)


@pytest.mark.parametrize("defect", Q.DEFECTS + ("kv_scales_swapped",))
def test_seeded_defects_fail_the_oracle_comparison(defect):
    """What the GPU tests compare (bytes and scales of K and V, bit for bit) must tell each defect apart."""
    g = torch.Generator().manual_seed(7)
    k = (torch.randn(3, 5, 2, 64, generator=g) * 3).bfloat16()  # [B, S, Hkv, D]
    v = torch.randn(3, 5, 2, 64, generator=g).bfloat16()
    want = Q.quantize(k) + Q.quantize(v)
    if defect == "kv_scales_swapped":
        got = (want[0], want[3], want[2], want[1])
    else:
        got = Q.quantize(k, defect) + Q.quantize(v, defect)
    assert not all(torch.equal(a, b) for a, b in zip(got, want))
    # ... and the edge rows alone tell rounding and exponent defects apart
    if defect in ("truncate", "e_plus_one", "e_minus_one"):
        e = Q.edge_rows(torch.bfloat16, 64)
        assert not all(torch.equal(a, b) for a, b in zip(Q.quantize(e, defect), Q.quantize(e)))


def test_e4m3_table_against_torch():
    """The oracle's table is OCP e4m3fn: every code decodes to torch's value, and encode inverts decode."""
    codes = torch.arange(256, dtype=torch.uint8)
    want = codes.view(torch.float8_e4m3fn).double()
    got = torch.from_numpy(Q.DECODE.copy())
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(got.nan_to_num(9.0), want.nan_to_num(9.0))
    fin = ~torch.isnan(got)
    assert torch.equal(torch.from_numpy(Q.e4m3_encode(Q.DECODE[fin.numpy()])), codes[fin])


# ---------------------------------------------------------------------------------------
def _model(preset="llama-micro", seq_len=64, seed=0, dtype=torch.float64, **kw):
    torch.manual_seed(seed)
    return Transformer(get_preset(preset, seq_len=seq_len, **kw)).to(dtype).eval()


@pytest.mark.parametrize("preset", ["llama-micro", "llama-tiny"])
def test_cache_size_and_layout(preset):
    a = get_preset(preset, seq_len=64)
    c16 = inf.KVCache(a, 3, 40, torch.bfloat16, "cpu")
    c8 = inf.KVCache(a, 3, 40, torch.bfloat16, "cpu", kv_dtype="fp8")
    D = a.head_dim
    assert c8.nbytes() * 2 * D == c16.nbytes() * (D + 4)
    assert c8.k[0].dtype == torch.uint8 and c8.k[0].shape == (3, 40, a.kv_heads, D)
    assert c8.k_scale[0].dtype == torch.float32 and c8.v_scale[0].shape == (3, 40, a.kv_heads)
    assert c16.k_scale[0] is None and c16.kv_dtype == "model" and c8.kv_dtype == "fp8"
    with pytest.raises(ValueError, match="kv_dtype"):
        inf.KVCache(a, 3, 40, torch.bfloat16, "cpu", kv_dtype="int8")


@pytest.mark.parametrize("preset", ["llama-micro", "llama-tiny"])
def test_fp64_model_steps_through_the_dequantized_cache(preset, monkeypatch):
    """prefill + decode_step with an fp8 cache equal the same model run with a cache in its own dtype that holds
    the oracle's dequantized rows: after the prefill, and after every append, the stored rows are replaced by
    dequantize(quantize(row)) before attention_decode_ref reads them. Ragged prompts (3 and 8 tokens)."""
    m = _model(preset)
    g = torch.Generator().manual_seed(2)
    toks = torch.randint(0, m.vocab_size, (2, 20), generator=g)
    lens = torch.tensor([3, 8])

    c8 = inf.KVCache(m.model_args, 2, 24, torch.float64, "cpu", kv_dtype="fp8")
    got = [inf.prefill(m, toks[:, :8], lens, c8)]
    for t in range(8, 20):
        got.append(inf.decode_step(m, toks[:, t], c8))

    def round_trip(x):
        return Q.dequantize(*Q.quantize(x))

    c = inf.KVCache(m.model_args, 2, 24, torch.float64, "cpu")
    want = [inf.prefill(m, toks[:, :8], lens, c)]
    for kc, vc in zip(c.k, c.v):
        kc[:, :8], vc[:, :8] = round_trip(kc[:, :8]), round_trip(vc[:, :8])
    real = inf.rope_append

    def append_then_round_trip(qkv, tab, kv_len, kc, vc, ks=None, vs=None):
        assert ks is None and vs is None
        real(qkv, tab, kv_len, kc, vc)
        bi, pos = torch.arange(2), kv_len.long()
        kc[bi, pos], vc[bi, pos] = round_trip(kc[bi, pos]), round_trip(vc[bi, pos])

    monkeypatch.setattr(inf, "rope_append", append_then_round_trip)
    for t in range(8, 20):
        want.append(inf.decode_step(m, toks[:, t], c))
    assert torch.equal(got[0], want[0])
    assert max((a - b).abs().max().item() for a, b in zip(got, want)) <= 1e-12
    assert c8.kv_len.tolist() == c.kv_len.tolist() == [15, 20]
    # the stored cache is the oracle applied to what the model-dtype cache would hold
    c16 = inf.KVCache(m.model_args, 2, 24, torch.float64, "cpu")
    inf.prefill(m, toks[:, :8], lens, c16)
    for i in range(len(c8.k)):
        for b, n in enumerate([3, 8]):
            q, s = Q.quantize(c16.k[i][b, :n])
            assert torch.equal(c8.k[i][b, :n], q) and torch.equal(c8.k_scale[i][b, :n], s)
            q, s = Q.quantize(c16.v[i][b, :n])
            assert torch.equal(c8.v[i][b, :n], q) and torch.equal(c8.v_scale[i][b, :n], s)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32, torch.bfloat16], ids=A.dname)
def test_first_token_logits_are_bit_equal_to_the_model_cache(dtype):
    m = _model("llama-micro", dtype=dtype)
    toks = torch.randint(0, m.vocab_size, (2, 9), generator=torch.Generator().manual_seed(4))
    lens = torch.tensor([9, 4])
    a = inf.prefill(m, toks, lens, inf.KVCache(m.model_args, 2, 16, dtype, "cpu"))
    c8 = inf.KVCache(m.model_args, 2, 16, dtype, "cpu", kv_dtype="fp8")
    b = inf.prefill(m, toks, lens, c8)
    assert torch.equal(a, b)
    # the next step reads dequantized keys: close to, and not equal to, the model cache's
    c = inf.KVCache(m.model_args, 2, 16, dtype, "cpu")
    inf.prefill(m, toks, lens, c)
    nxt, nxt8 = inf.decode_step(m, toks[:, 0], c), inf.decode_step(m, toks[:, 0], c8)
    assert not torch.equal(nxt, nxt8)
    assert (nxt.double() - nxt8.double()).abs().max().item() < 0.25 * nxt.double().abs().max().item()


def test_cache_kind_is_checked():
    m = _model("llama-micro")
    toks = torch.zeros(2, 4, dtype=torch.long)
    with pytest.raises(ValueError, match="KVCache is"):
        inf.prefill(m, toks, torch.tensor([4, 4]), inf.KVCache(m.model_args, 2, 8, torch.float32, "cpu", kv_dtype="fp8"))
    c8 = inf.KVCache(m.model_args, 2, 8, torch.float64, "cpu", kv_dtype="fp8")
    c8.k_scale[0] = c8.k_scale[0][:, :4]
    with pytest.raises(ValueError, match="fp8 cache holds"):
        inf.prefill(m, toks, torch.tensor([4, 4]), c8)


def test_generate_with_an_fp8_cache_and_invalid_combinations():
    m = _model("llama-tiny")
    prompts = [[5, 9, 2], [7, 1, 4, 4, 8, 3, 11, 6]]
    base, _ = inf.generate(m, prompts, 12)
    got, why = inf.generate(m, prompts, 12, kv_cache_dtype="fp8")
    assert why == ["max_new_tokens"] * 2 and [len(t) for t in got] == [12, 12]
    assert [t[0] for t in got] == [t[0] for t in base]  # the prompt's attention is unquantized
    again, _ = inf.generate(m, prompts, 12, kv_cache_dtype="fp8", sampler="philox")
    assert again == got  # greedy under either sampler
    with pytest.raises(ValueError, match="needs the KV cache"):
        inf.generate(m, prompts, 4, kv_cache_dtype="fp8", use_cache=False)
    with pytest.raises(ValueError, match="kv_cache_dtype"):
        inf.generate(m, prompts, 4, kv_cache_dtype="e5m2")


@pytest.mark.parametrize("dtype", DTYPES, ids=A.dname)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Hq,Hkv", Q.GROUPS)
def test_decode_reference_with_one_rounding_is_within_the_cap(Hq, Hkv, D, dtype):
    """attention_decode_fp8_ref (fp32 math on the dequantized cache) with o rounded once to the storage dtype:
    rho <= cap(dtype, "decode_o") and lse within lse_bound on the cases of the GPU test."""
    bad = []
    for name in Q.RECIPES:
        c = Q.decode_case(name, D, dtype, Hq, Hkv)
        o, lse = ref.attention_decode_fp8_ref(c.q[:, 0], c.kq, c.vq, c.ks, c.vs, c.kv_len, c.scale)
        assert o.dtype == torch.float32
        r, i = A.rho(o.to(dtype)[:, None], c.o, c.m_o)
        el = float((lse.double()[:, :, None] - c.lse).abs().max())
        print(f"{name} D={D} {A.dname(dtype)} G={Hq // Hkv}: rho/u = {r / A.unit(dtype):.3f} lse err {el:.2e}")
        if not (r <= A.cap(dtype, "decode_o") and el <= c.lse_bound):
            bad.append((name, r / A.unit(dtype), i, el, c.lse_bound))
    assert not bad, bad


def test_decode_reference_ignores_the_tail_and_handles_length_zero():
    c = Q.decode_case("peaked", 64, torch.bfloat16, 4, 2)
    kq, vq, ks, vs = c.kq.clone(), c.vq.clone(), c.ks.clone(), c.vs.clone()
    n = torch.tensor([0, 255, 256, 257, 785], dtype=torch.int32)
    base = ref.attention_decode_fp8_ref(c.q[:, 0], kq, vq, ks, vs, n, c.scale)
    for b, L in enumerate(n.tolist()):
        kq[b, L:], vq[b, L:] = 0x7F, 0x7F
        ks[b, L:], vs[b, L:] = float("nan"), float("nan")
    o, lse = ref.attention_decode_fp8_ref(c.q[:, 0], kq, vq, ks, vs, n, c.scale)
    assert torch.equal(o, base[0]) and torch.equal(lse, base[1])
    assert bool((o[0] == 0).all()) and bool(torch.isneginf(lse[0]).all()) and bool(torch.isfinite(o).all())


# ---------------------------------------------------------------------------------------
def test_generate_cli_records_the_cache_dtype(tmp_path):
    from pyrecover_amd import _ext

    if not _ext.available():
        pytest.skip("native extension not built (the checkpoint writer is native)")
    from tests.test_generate import _trained

    _trained(tmp_path, False)
    common = [sys.executable, os.path.join(ROOT, "generate.py"), "--checkpoint-dir", str(tmp_path), "--model-preset",
              "llama-micro", "--sequence-length", "32", "--model-dtype", "fp64", "--prompt-tokens", "3,4,5",
              "--prompt-tokens", "9,8,7,6,5", "--max-new-tokens", "8"]
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    first = {}
    for kind in ("fp8", "model"):
        out = tmp_path / f"{kind}.jsonl"
        r = subprocess.run(common + ["--kv-cache-dtype", kind, "--output-jsonl", str(out)], capture_output=True,
                           text=True, env=env, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        recs = [json.loads(line) for line in out.read_text().splitlines()]
        assert [rec["kv_cache_dtype"] for rec in recs] == [kind] * 2
        assert all(len(rec["generated_ids"]) == 8 for rec in recs)
        first[kind] = [rec["generated_ids"][0] for rec in recs]
    assert first["fp8"] == first["model"]
    r = subprocess.run(common + ["--kv-cache-dtype", "fp8", "--no-kv-cache"], capture_output=True, text=True, env=env,
                       timeout=300)
    assert r.returncode != 0 and "needs the KV cache" in r.stderr
    r = subprocess.run(common + ["--kv-cache-dtype", "int4"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode != 0 and "invalid choice" in r.stderr
