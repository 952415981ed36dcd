"""Paged KV cache on the GPU (csrc/kernels/attention_paged.hip): every paged kernel against its dense counterpart
on the gathered cache, bit for bit, and against the fp32 torch oracle; the model-level paths against the dense
cache's tokens and logits."""
import math

import pytest
import torch

from pyrecover_amd import _ext
from pyrecover_amd import inference as inf
from pyrecover_amd.config import get_preset
from pyrecover_amd.models.llama import Transformer
from pyrecover_amd.ops import reference as R

pytestmark = pytest.mark.gpu

O_TOL, LSE_TOL = 2e-2, 1e-3  # bounds of test_kernels_gpu.py::test_attention_fwd
CAP = 400
PAGES = [64, 128, 256]


def _lens(cuda, lens):
    return torch.tensor(lens, device=cuda, dtype=torch.int32)


def _bits(x):
    return x.contiguous().view(torch.int16)  # NaN pages compare equal as bits


def _paged(k, v, page, need, extra=3):
    """The dense k, v [B, cap, Hkv, D] scattered into pools through a random permutation of page ids: sequence b
    maps the pages of its first need[b] tokens, every other table entry is -1, and `extra` pages that no table
    names hold NaN (k) / Inf (v), as do pool rows past cap."""
    B, cap = k.shape[:2]
    npg = [-(-n // page) for n in need]
    ids = torch.randperm(sum(npg) + extra, generator=torch.Generator().manual_seed(page)).tolist()
    kp = torch.full((len(ids), page) + tuple(k.shape[2:]), float("nan"), dtype=k.dtype, device=k.device)
    vp = torch.full_like(kp, float("inf"))
    bt = torch.full((B, -(-cap // page)), -1, dtype=torch.int32)
    for b in range(B):
        for i in range(npg[b]):
            bt[b, i] = pid = ids.pop()
            rows = slice(i * page, min((i + 1) * page, cap))
            kp[pid, :rows.stop - rows.start], vp[pid, :rows.stop - rows.start] = k[b, rows], v[b, rows]
    return kp, vp, bt.to(k.device)


def _inputs(cuda, B, T, Hq, Hkv, D, dtype, seed=0):
    """test_extend_gpu.py::_inputs: standard normal, q the strided view of a fused QKV activation."""
    torch.manual_seed(seed)
    qkv = torch.randn(B * T, (Hq + 2 * Hkv) * D, device=cuda).to(dtype)
    k = torch.randn(B, CAP, Hkv, D, device=cuda).to(dtype)
    v = torch.randn(B, CAP, Hkv, D, device=cuda).to(dtype)
    return qkv[:, :Hq * D].view(B, T, Hq, D), k, v


def _close(o, lse, o_ref, lse_ref):
    eo = (o.float() - o_ref).abs().max().item()
    el = (lse - lse_ref).abs().masked_fill(lse == lse_ref, 0).max().item()  # an empty cache: -inf on both sides
    print(f"|o - o_ref| = {eo:.3e}, |lse - lse_ref| = {el:.3e}")
    assert eo < O_TOL and el < LSE_TOL


@pytest.mark.parametrize("page", PAGES)
@pytest.mark.parametrize("Hq,Hkv", [(2, 2), (4, 1), (8, 1)])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_attn_decode_paged(cuda, dtype, D, Hq, Hkv, page):
    """An empty cache and both sides of a page, a tile and a chunk boundary."""
    C, scale = _ext.native(), 1 / math.sqrt(D)
    kv_len = [0, 1, 63, 64, 65, 255, 256, 257, 399]
    q, k, v = _inputs(cuda, len(kv_len), 1, Hq, Hkv, D, dtype)
    q, n = q[:, 0], _lens(cuda, kv_len)
    kp, vp, bt = _paged(k, v, page, kv_len)
    o, lse = C.attn_decode_paged(q, kp, vp, bt, n, CAP, scale)
    kd, vd = R.paged_gather(kp, bt, CAP), R.paged_gather(vp, bt, CAP)
    od, ld = C.attn_decode(q, kd, vd, n, scale)
    assert torch.equal(o, od) and torch.equal(lse, ld)
    _close(o, lse, *R.attention_decode_ref(q.float(), k.float(), v.float(), n, scale))


def _extend_case(cuda, T, split, page, Hq, Hkv, D, dtype, base):
    C, scale = _ext.native(), 1 / math.sqrt(D)
    q, k, v = _inputs(cuda, len(base), T, Hq, Hkv, D, dtype, seed=1)
    n = _lens(cuda, base)
    kp, vp, bt = _paged(k, v, page, [min(CAP, max(b, 0) + T) for b in base])
    o, lse = C.attn_extend_paged(q, kp, vp, bt, n, CAP, scale, split)
    kd, vd = R.paged_gather(kp, bt, CAP), R.paged_gather(vp, bt, CAP)
    od, ld = C.attn_extend(q, kd, vd, n, scale, split)
    assert torch.equal(o, od) and torch.equal(lse, ld)
    _close(o, lse, *R.attention_extend_ref(q.float(), k.float(), v.float(), n, scale))


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Hq,Hkv", [(2, 2), (8, 1)])
@pytest.mark.parametrize("page", PAGES)
@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("T", [1, 5, 33, 135])
def test_attn_extend_paged(cuda, T, split, page, Hq, Hkv, D):
    _extend_case(cuda, T, split, page, Hq, Hkv, D, torch.bfloat16, [0, 1, 63, 64, 200])


@pytest.mark.parametrize("split", [0, 1])
def test_attn_extend_paged_fp16_and_overflow(cuda, split):
    """fp16, and kv_len + T > cap (also kv_len outside [0, cap]): the dense kernel's clamps, bit for bit."""
    _extend_case(cuda, 33, split, 128, 8, 1, 128, torch.float16, [0, 1, 63, 64, 200])
    _extend_case(cuda, 33, split, 64, 4, 2, 64, torch.bfloat16, [CAP - 10, CAP + 5, -3, CAP - 33])


def _mapped_rows(kp, bt, cap):
    """(flat pool row [B, cap], mapped [B, cap]) of every logical position."""
    page = kp.shape[1]
    j = torch.arange(cap, device=kp.device)
    e = bt.long()[:, j // page]
    return e.clamp(min=0) * page + j % page, e >= 0


@pytest.mark.parametrize("page", [64, 128])
@pytest.mark.parametrize("T", [1, 33])
def test_rope_append_paged(cuda, T, page):
    """Appends that cross a page boundary (T = 33 from page - 8), land on a page's last and first row (T = 1), and
    one sequence whose next page is -1: it stores nothing there, its q is rotated all the same. Pools and q
    bit-equal to the dense rope_append_ on the gather; every other pool row, NaN pages included, untouched."""
    C = _ext.native()
    D, Hq, Hkv, B = 64, 4, 2, 4
    base = [page - 1, 0, 5, page] if T == 1 else [page - 8, 0, 5, page - 8]
    need = [base[0] + T, T, 5 + T, page]  # the last sequence owns one page only
    torch.manual_seed(2)
    tab = R.rope_table(R.precompute_freqs_cis(D, CAP)).to(cuda)
    qkv = torch.randn(B * T, (Hq + 2 * Hkv) * D, device=cuda).bfloat16()
    k, v = (torch.randn(B, CAP, Hkv, D, device=cuda).bfloat16() for _ in range(2))
    kp, vp, bt = _paged(k, v, page, need)
    kd, vd = R.paged_gather(kp, bt, CAP), R.paged_gather(vp, bt, CAP)
    rows, ok = _mapped_rows(kp, bt, CAP)
    want_k, want_v = kp.clone().view(-1, Hkv, D), vp.clone().view(-1, Hkv, D)
    qd, qp, n = qkv.clone(), qkv.clone(), _lens(cuda, base)
    C.rope_append_(qd, tab, n, kd, vd)
    C.rope_append_paged_(qp, tab, n, kp, vp, bt, CAP)
    assert torch.equal(qp, qd)
    stored = 0
    for b in range(B):
        for p in range(base[b], base[b] + T):
            if ok[b, p]:
                want_k[rows[b, p]], want_v[rows[b, p]] = kd[b, p], vd[b, p]
                stored += 1
    assert stored == (3 * T if T == 1 else 3 * T + 8)  # the last sequence: nothing at T = 1, 8 rows of 33
    assert torch.equal(_bits(kp), _bits(want_k).view_as(_bits(kp)))
    assert torch.equal(_bits(vp), _bits(want_v).view_as(_bits(vp)))


def test_kv_store_paged(cuda):
    """S = 200 prompt rows into sequences reserved for 200 and for 70 tokens: the mapped rows hold the source,
    the padding beyond the second sequence's two pages went nowhere, nothing else in the pool changed."""
    C = _ext.native()
    D, Hq, Hkv, B, S, page = 128, 4, 2, 2, 200, 64
    torch.manual_seed(3)
    qkv = torch.randn(B * S, (Hq + 2 * Hkv) * D, device=cuda).bfloat16()
    ks = qkv[:, Hq * D:(Hq + Hkv) * D].view(B, S, Hkv, D)
    vs = qkv[:, (Hq + Hkv) * D:].view(B, S, Hkv, D)
    k0, v0 = (torch.randn(B, CAP, Hkv, D, device=cuda).bfloat16() for _ in range(2))
    kp, vp, bt = _paged(k0, v0, page, [200, 70])
    rows, ok = _mapped_rows(kp, bt, CAP)
    want_k, want_v = kp.clone().view(-1, Hkv, D), vp.clone().view(-1, Hkv, D)
    sel = ok[:, :S]
    assert sel.sum().item() == 200 + 128
    want_k[rows[:, :S][sel]], want_v[rows[:, :S][sel]] = ks[sel], vs[sel]
    C.kv_store_paged_(ks, vs, kp, vp, bt, CAP)
    assert torch.equal(_bits(kp), _bits(want_k).view_as(_bits(kp)))
    assert torch.equal(_bits(vp), _bits(want_v).view_as(_bits(vp)))
    assert torch.equal(R.paged_gather(kp, bt, CAP)[:, :S][sel], ks[sel])


def test_paged_bindings_reject_bad_arguments(cuda):
    C = _ext.native()
    D, Hq, Hkv = 64, 4, 2
    q, k, v = _inputs(cuda, 2, 1, Hq, Hkv, D, torch.bfloat16)
    q, n = q[:, 0], _lens(cuda, [70, 3])
    kp, vp, bt = _paged(k, v, 64, [70, 3])
    C.attn_decode_paged(q, kp, vp, bt, n, CAP, 0.125)  # the good call
    bad = [
        ("page size", (q, torch.zeros(3, 96, Hkv, D, device=cuda).bfloat16(),
                       torch.zeros(3, 96, Hkv, D, device=cuda).bfloat16(), bt, n)),
        ("int32", (q, kp, vp, bt.long(), n)),
        ("block_table must be", (q, kp, vp, bt[:, :-1].contiguous(), n)),
        ("must be on", (q, kp, vp, bt.cpu(), n)),
        ("dtype", (q, kp.half(), vp.half(), bt, n)),
    ]
    for match, args in bad:
        with pytest.raises(RuntimeError, match=match):
            C.attn_decode_paged(*args, CAP, 0.125)
        with pytest.raises(RuntimeError, match=match):
            C.attn_extend_paged(args[0].unsqueeze(1), *args[1:], CAP, 0.125)
    q96 = torch.randn(2, Hq, 96, device=cuda).bfloat16()
    p96 = torch.zeros(kp.shape[0], 64, Hkv, 96, device=cuda).bfloat16()
    with pytest.raises(RuntimeError, match="head_dim"):
        C.attn_decode_paged(q96, p96, p96.clone(), bt, n, CAP, 0.1)
    tab = R.rope_table(R.precompute_freqs_cis(D, CAP)).to(cuda)
    qkv = torch.randn(2, (Hq + 2 * Hkv) * D, device=cuda).bfloat16()
    with pytest.raises(RuntimeError, match="int32"):
        C.rope_append_paged_(qkv, tab, n, kp, vp, bt.long(), CAP)
    with pytest.raises(RuntimeError, match="block_table must be"):
        C.kv_store_paged_(k[:, :8], v[:, :8], kp, vp, bt, CAP + 64)


# ---------------------------------------------------------------------------------------
def _model(cuda):
    torch.manual_seed(0)
    cfg = get_preset("llama-micro", seq_len=128)  # head_dim 64, GQA 2:1
    return cfg, Transformer(cfg).to(cuda).bfloat16().eval()


@pytest.mark.parametrize("kw", [{}, {"prefill_chunk": 32}, {"graph": True}], ids=["plain", "chunked", "graph"])
def test_generate_paged_matches_dense(cuda, kw):
    """Greedy, ragged prompts: the paged cache returns the dense cache's tokens and finish reasons (the kernels
    return its bits) from fewer bytes; the hipGraph loop replays over the static table."""
    cfg, m = _model(cuda)
    g = torch.Generator().manual_seed(1)
    prompts = [torch.randint(0, cfg.vocab_size, (n,), generator=g).tolist() for n in (3, 70, 17)]
    sd, sp = {}, {}
    dense = inf.generate(m, prompts, 20, stats=sd, **kw)
    paged = inf.generate(m, prompts, 20, stats=sp, kv_page_size=64, **kw)
    assert paged == dense
    assert 0 < sp["kv_cache_bytes"] < sd["kv_cache_bytes"]
    if kw.get("graph"):
        assert sp["graph_replays"] > 0


def test_share_prefix_logits(cuda):
    """Row 1 shares row 0's 70-token prefix (one full page of 64 named twice, the partial page copied), then
    both rows append different tokens: extend and a further decode_step give, on both rows, the logits of a
    dense cache whose rows were prefilled independently, bit for bit. So neither row's appends reach the other."""
    cfg, m = _model(cuda)
    g = torch.Generator().manual_seed(2)
    n, T = 70, 9
    prompt = torch.randint(0, cfg.vocab_size, (1, n), generator=g).to(cuda).expand(2, n).contiguous()
    new = torch.randint(0, cfg.vocab_size, (2, T + 1), generator=g).to(cuda)
    lens, nn = torch.full((2,), n, device=cuda), torch.full((2,), T, device=cuda)
    dense = inf.KVCache(cfg, 2, 128, torch.bfloat16, cuda)
    want = [inf.prefill(m, prompt, lens, dense), inf.extend(m, new[:, :T], nn, dense),
            inf.decode_step(m, new[:, T], dense)]
    cache = inf.PagedKVCache(cfg, 2, 128, torch.bfloat16, cuda, page_size=64, n_pages=5)
    cache.reserve(0, n + T + 1)
    got = [inf.prefill(m, prompt, lens, cache)]  # row 1 owns no page yet: its rows go nowhere
    cache.share_prefix(0, 1, n)
    cache.reserve(1, n + T + 1)
    assert cache.pages_in_use() == 3 and cache.kv_len.tolist() == [n, n]
    got += [inf.extend(m, new[:, :T], nn, cache), inf.decode_step(m, new[:, T], cache)]
    for a, b in zip(got, want):
        assert torch.equal(a, b)
