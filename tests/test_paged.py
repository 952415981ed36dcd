"""Paged KV cache on the CPU: the reference math of ops/reference.py, the PagedKVCache allocator and the
torch-math generation path."""
import warnings

import pytest
import torch

from pyrecover_amd import inference as inf
from pyrecover_amd.config import get_preset
from pyrecover_amd.models.llama import Transformer
from pyrecover_amd.ops import reference as R

CAP, PAGE, HKV, D = 150, 64, 2, 8


def _pools():
    """Dense fp64 caches [3, CAP, HKV, D] and their pools under a shuffled table; sequence 2's last entries are
    -1 and an out-of-range id, whose keys are therefore zeros. The pages no table names, and pool rows past CAP, hold NaN."""
    torch.manual_seed(0)
    k, v = torch.randn(3, CAP, HKV, D, dtype=torch.float64), torch.randn(3, CAP, HKV, D, dtype=torch.float64)
    bt = torch.tensor([[7, 2, 5], [0, 8, 3], [6, -1, 11]], dtype=torch.int32)
    k[2, PAGE:], v[2, PAGE:] = 0, 0
    kp, vp = (torch.full((10, PAGE, HKV, D), float("nan"), dtype=torch.float64) for _ in range(2))
    for b in range(3):
        for i, pid in enumerate(bt[b].tolist()):
            if 0 <= pid < 10:
                n = min(PAGE, CAP - i * PAGE)
                kp[pid, :n], vp[pid, :n] = k[b, i * PAGE:i * PAGE + n], v[b, i * PAGE:i * PAGE + n]
    return k, v, kp, vp, bt


def test_paged_refs_are_the_dense_refs_on_the_gather():
    k, v, kp, vp, bt = _pools()
    assert torch.equal(R.paged_gather(kp, bt, CAP), k) and torch.equal(R.paged_gather(vp, bt, CAP), v)
    q = torch.randn(3, 5, 4, D, dtype=torch.float64)
    n = torch.tensor([0, 149, 40])
    for a, b in zip(R.attention_decode_paged_ref(q[:, 0], kp, vp, bt, n, CAP), R.attention_decode_ref(q[:, 0], k, v, n)):
        assert torch.equal(a, b)
    for a, b in zip(R.attention_extend_paged_ref(q, kp, vp, bt, n, CAP), R.attention_extend_ref(q, k, v, n)):
        assert torch.equal(a, b)
    # the append and the prompt store: the dense result over the mapped rows, nothing on the unmapped pages
    tab = R.rope_table(R.precompute_freqs_cis(D, CAP))
    qkv = torch.randn(3 * 5, (4 + 2 * HKV) * D, dtype=torch.float64)
    base = torch.tensor([62, 147, 61])  # across a page, past the capacity, onto an unmapped page
    qd, qp, nan0 = qkv.clone(), qkv.clone(), kp.isnan().sum().item()
    R.rope_append_ref(qd, tab, base, k, v)
    R.rope_append_paged_ref(qp, tab, base, kp, vp, bt, CAP)
    k[2, PAGE:], v[2, PAGE:] = 0, 0  # what the dense append wrote where sequence 2 has no page
    assert torch.equal(qp, qd) and kp.isnan().sum().item() == nan0
    assert torch.equal(R.paged_gather(kp, bt, CAP), k) and torch.equal(R.paged_gather(vp, bt, CAP), v)
    ks, vs = torch.randn(3, 100, HKV, D, dtype=torch.float64), torch.randn(3, 100, HKV, D, dtype=torch.float64)
    R.kv_store_paged_ref(ks, vs, kp, vp, bt, CAP)
    ks[2, PAGE:], vs[2, PAGE:] = 0, 0
    assert torch.equal(R.paged_gather(kp, bt, CAP)[:, :100], ks) and torch.equal(R.paged_gather(vp, bt, CAP)[:, :100], vs)
    assert kp.isnan().sum().item() == nan0


def test_allocator():
    cfg = get_preset("llama-micro", seq_len=256)
    c = inf.PagedKVCache(cfg, 3, 200, torch.float32, "cpu", page_size=64, n_pages=5)
    assert c.block_table.shape == (3, 4) and (c.block_table == -1).all() and c.pages_in_use() == 0
    c.reserve(0, 70)
    row = c.block_table[0].tolist()
    c.reserve(0, 70), c.reserve(0, 10)  # idempotent, grows only
    assert c.block_table[0].tolist() == row and row[2:] == [-1, -1] and c.pages_in_use() == 2
    c.reserve(0, 129)
    assert c.block_table[0].tolist()[:2] == row[:2] and c.pages_in_use() == 3
    with pytest.raises(RuntimeError, match="short by 1"):
        c.reserve(1, 192)
    assert c.pages_in_use() == 3 and (c.block_table[1] == -1).all()  # a failed reserve maps nothing
    # share 100 tokens: page 0 named twice, the partial page copied into a fresh one
    c.k[1][row[1], :36] = 7.0
    c.share_prefix(0, 1, 100)
    t1 = c.block_table[1].tolist()
    assert t1[0] == row[0] and t1[1] not in row and t1[2:] == [-1, -1] and c.kv_len.tolist() == [0, 100, 0]
    assert (c.k[1][t1[1], :36] == 7.0).all() and c.pages_in_use() == 4
    c.release(0)  # the shared page survives its first owner
    assert c.pages_in_use() == 2 and (c.block_table[0] == -1).all() and c.block_table[1].tolist() == t1
    c.release(1)
    assert c.pages_in_use() == 0 and c.nbytes() == 2 * 2 * 5 * 64 * 1 * 64 * 4 + 3 * 4 * 4
    c.reserve(2, 200), c.reserve(1, 64)  # every page is back
    assert c.pages_in_use() == 5


def test_generate_paged_on_cpu_and_refusals():
    torch.manual_seed(0)
    cfg = get_preset("llama-micro", seq_len=128)
    m = Transformer(cfg).float().eval()
    g = torch.Generator().manual_seed(1)
    prompts = [torch.randint(0, cfg.vocab_size, (n,), generator=g).tolist() for n in (3, 70, 17)]
    sd, sp = {}, {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # the once-per-shape note of the torch-math path
        dense = inf.generate(m, prompts, 20, stats=sd)
        assert inf.generate(m, prompts, 20, stats=sp, kv_page_size=64) == dense
        assert (inf.generate(m, prompts, 20, kv_page_size=64, prefill_chunk=32) ==
                inf.generate(m, prompts, 20, prefill_chunk=32))
    assert 0 < sp["kv_cache_bytes"] < sd["kv_cache_bytes"]
    for kw in ({"kv_page_size": 100}, {"kv_page_size": 64, "use_cache": False},
               {"kv_page_size": 64, "kv_cache_dtype": "fp8"}):
        with pytest.raises(ValueError, match="kv_page_size"):
            inf.generate(m, prompts, 4, **kw)
    with pytest.raises(ValueError, match="follow-up"):
        inf.PagedKVCache(cfg, 1, 64, torch.float32, "cpu", kv_dtype="fp8")
    with pytest.raises(ValueError, match="page_size"):
        inf.PagedKVCache(cfg, 1, 64, torch.float32, "cpu", page_size=100)
