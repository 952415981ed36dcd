"""Shared-prefix decode attention on the GPU (csrc/kernels/attention_decode_shared.hip): attn_decode_shared_paged
against the fp32 torch oracle on each sequence's logical dense cache, its bit contracts, the binding's refusals,
and the model-level paths (fork + decode_step, generate(n_samples=N))."""
import math

import pytest
import torch

from pyrecover_amd import _ext
from pyrecover_amd import inference as inf
from pyrecover_amd.config import get_preset
from pyrecover_amd.models.llama import Transformer
from pyrecover_amd.ops import reference as R
from tests.test_generate_gpu import _ref_forward

pytestmark = pytest.mark.gpu

O_TOL, LSE_TOL = 2e-2, 1e-3  # bounds of test_paged_gpu.py, from test_kernels_gpu.py::test_attention_fwd
CAP = 700                    # chunks 0-255, 256-511, 512-699
# shared_len of a group (320 rounds down, 900 clamps to CAP) -> the kv_len its members cycle through. Short members in
# designated groups only: 0 empties group 320, 511 lowers group 900 to one chunk; 256 and 512 keep s_eff at every n.
LENS = {0: [0, 1, 511, 512, 513, 699], 256: [256, 257, 511, 512, 513, 699], 320: [256, 0, 257, 511, 512, 513, 699],
        512: [512, 513, 699], 900: [699, 511, 513, 512]}
SHARED = list(LENS)


def _case(cuda, dtype, D, Hq, Hkv, page, n, perm=0, shared=SHARED):
    """len(shared) groups of n sequences. The members of group g hold the same keys and name the same shuffled
    pages for the pages that shared[g] tokens touch, and keys and pages of their own after them; pages that no
    table names, and pool rows past CAP, hold NaN (k) / Inf (v). Member i of a group has kv_len
    LENS[shared_len][i % len]: s_eff, s_eff + 1, 511, 512, 513, 699 and 0, some shorter than shared_len."""
    B, P = n * len(shared), -(-CAP // page)
    torch.manual_seed(0)
    q = torch.randn(B, Hq, D, device=cuda).to(dtype)
    k, v = (torch.randn(B, P * page, Hkv, D, device=cuda).to(dtype) for _ in range(2))
    ids = torch.randperm(B * P + 3, generator=torch.Generator().manual_seed(page + perm))[:B * P].view(B, P)
    kv_len = []
    for g, sl in enumerate(shared):
        ns = -(-min(sl, CAP) // page)  # pages the group shares
        r0 = g * n
        k[r0 + 1:r0 + n, :ns * page], v[r0 + 1:r0 + n, :ns * page] = k[r0, :ns * page], v[r0, :ns * page]
        ids[r0 + 1:r0 + n, :ns] = ids[r0, :ns]
        kv_len += [LENS[sl][i % len(LENS[sl])] for i in range(n)]
    k[:, CAP:], v[:, CAP:] = float("nan"), float("inf")
    kp = torch.full((B * P + 3, page, Hkv, D), float("nan"), dtype=dtype, device=cuda)
    vp = torch.full_like(kp, float("inf"))
    flat = ids.view(-1).to(cuda)
    kp[flat], vp[flat] = k.view(B * P, page, Hkv, D), v.view(B * P, page, Hkv, D)  # shared pages: the same rows
    ints = lambda x: torch.tensor(x, dtype=torch.int32, device=cuda)  # noqa: E731
    return q, k[:, :CAP], v[:, :CAP], kp, vp, ids.to(torch.int32).to(cuda), ints(kv_len), ints(shared)


@pytest.mark.parametrize("n", [1, 3, 8, 40])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("Hq,Hkv", [(2, 2), (8, 1)])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("page", [64, 256])
def test_attn_decode_shared_vs_reference(cuda, page, D, Hq, Hkv, dtype, n):
    """R = n * Hq / Hkv rows from 1 to 320: every wave split and more than one row tile, each with groups that
    the shared kernel serves (s_eff, recomputed here on the host, is 256, 512 and >= 256 in three of them)."""
    C, scale = _ext.native(), 1 / math.sqrt(D)
    q, k, v, kp, vp, bt, kv_len, sl = _case(cuda, dtype, D, Hq, Hkv, page, n)
    s_eff = (torch.minimum(kv_len.view(-1, n).amin(1), sl.clamp(max=CAP)) // 256 * 256).tolist()
    assert s_eff[0] == 0 and s_eff[1] == 256 and s_eff[3] == 512 and s_eff[4] == (512 if n == 1 else 256)
    assert s_eff[2] == (256 if n == 1 else 0)
    o, lse = C.attn_decode_shared_paged(q, kp, vp, bt, kv_len, sl, n, CAP, scale)
    o_ref, lse_ref = R.attention_decode_ref(q.float(), k.float(), v.float(), kv_len, scale)
    eo = (o.float() - o_ref).abs().max().item()
    el = (lse - lse_ref).abs().masked_fill(lse == lse_ref, 0).max().item()  # an empty cache: -inf on both sides
    print(f"|o - o_ref| = {eo:.3e}, |lse - lse_ref| = {el:.3e}")
    assert eo < O_TOL and el < LSE_TOL


@pytest.mark.parametrize("D,Hq,Hkv,page,n", [(128, 8, 1, 64, 3), (64, 2, 2, 256, 40), (64, 8, 1, 64, 40)])
def test_attn_decode_shared_bits(cuda, D, Hq, Hkv, page, n):
    C, scale = _ext.native(), 1 / math.sqrt(D)
    q, _, _, kp, vp, bt, kv_len, sl = _case(cuda, torch.bfloat16, D, Hq, Hkv, page, n)
    o, lse = C.attn_decode_shared_paged(q, kp, vp, bt, kv_len, sl, n, CAP, scale)
    # nothing shared: the per-sequence kernel does everything, and returns attn_decode_paged's bits
    for a, b in zip(C.attn_decode_shared_paged(q, kp, vp, bt, kv_len, torch.zeros_like(sl), n, CAP, scale),
                    C.attn_decode_paged(q, kp, vp, bt, kv_len, CAP, scale)):
        assert torch.equal(a, b)
    for a, b in zip(C.attn_decode_shared_paged(q, kp, vp, bt, kv_len, sl, n, CAP, scale), (o, lse)):  # run to run
        assert torch.equal(a, b)
    rows = slice(3 * n, 4 * n)  # a group alone (group 3: two shared chunks) and inside the batch
    for a, b in zip(C.attn_decode_shared_paged(q[rows], kp, vp, bt[rows].contiguous(), kv_len[rows], sl[3:4], n, CAP,
                                               scale), (o, lse)):
        assert torch.equal(a, b[rows])
    q2, _, _, kp2, vp2, bt2, _, _ = _case(cuda, torch.bfloat16, D, Hq, Hkv, page, n, perm=1)  # other physical pages
    assert torch.equal(q2, q) and not torch.equal(bt2, bt)
    for a, b in zip(C.attn_decode_shared_paged(q, kp2, vp2, bt2, kv_len, sl, n, CAP, scale), (o, lse)):
        assert torch.equal(a, b)


def test_attn_decode_shared_binding_refusals(cuda):
    C = _ext.native()
    q, _, _, kp, vp, bt, kv_len, sl = _case(cuda, torch.bfloat16, 64, 2, 2, 64, 2, shared=[0, 256, 512])
    for match, s, n in [("group_size must be >= 1", sl, 0), ("must divide the batch", sl, 4),
                        ("shared_len must be", sl.long(), 2), ("shared_len must be", sl[:2], 2),
                        ("must be on", sl.cpu(), 2)]:
        with pytest.raises(RuntimeError, match=match):
            C.attn_decode_shared_paged(q, kp, vp, bt, kv_len, s, n, CAP, 0.125)


def _models(cuda, seq_len):
    torch.manual_seed(0)
    cfg = get_preset("llama-micro", seq_len=seq_len)  # head_dim 64, GQA 2:1
    m32 = Transformer(cfg).to(cuda).eval()
    m = Transformer(cfg).to(cuda)
    m.load_state_dict(m32.state_dict())
    m = m.bfloat16().eval()
    m32.load_state_dict(m.state_dict())  # the same (bf16-representable) weights in fp32
    return cfg, m, m32


def test_forked_decode_logits_vs_fp32_model(cuda):
    """Teacher-forced, bf16: a 300-token prompt prefilled once, fork(3), then 8 decode steps with other tokens on
    every sibling (one shared chunk of 256 keys, the rest per sequence). With e_full / e_shared the max abs error
    of the HIP full-forward / forked decode-path logits against the fp32 plain-torch model on the same rows
    (299 .. 307), require e_shared <= 2 * e_full + 1e-3: the rule and floor of test_decode_logits_vs_fp32_model."""
    cfg, m, m32 = _models(cuda, 512)
    P, N, n = 300, 8, 3
    tok = torch.randint(0, cfg.vocab_size, (n, P + N), device=cuda)
    tok[:, :P] = tok[0, :P]
    with torch.no_grad():
        ref = _ref_forward(m32, tok)[:, P - 1:P + N]
        full = m(tok).float()[:, P - 1:P + N]
        cache = inf.PagedKVCache(cfg, 1, P + N, torch.bfloat16, cuda, page_size=64, n_pages=7)
        cache.reserve(0, P + N)
        rows = [inf.prefill(m, tok[:1, :P], torch.full((1,), P, device=cuda), cache).expand(n, -1)]
        cache = cache.fork(n, [P])
        for b in range(n):
            cache.reserve(b, P + N)
        assert cache.shared_len.tolist() == [256] and cache.pages_in_use() == 7
        for t in range(P, P + N):
            rows.append(inf.decode_step(m, tok[:, t], cache))
    dec = torch.stack(rows, 1).float()
    e_full, e_shared = (full - ref).abs().max().item(), (dec - ref).abs().max().item()
    print(f"e_full = {e_full:.3e}, e_shared = {e_shared:.3e}")
    assert cache.kv_len.tolist() == [P + N] * n
    assert e_shared <= 2 * e_full + 1e-3


@pytest.mark.parametrize("graph", [False, True])
def test_generate_n_samples(cuda, graph):
    """Greedy: the three samples of a prompt are the same tokens, from fewer bytes than three copies of it."""
    cfg, m, _ = _models(cuda, 512)
    g = torch.Generator().manual_seed(1)
    prompts = [torch.randint(0, cfg.vocab_size, (n,), generator=g).tolist() for n in (3, 70, 300)]
    s3, s1 = {}, {}
    tokens, reasons = inf.generate(m, prompts, 12, kv_page_size=64, n_samples=3, graph=graph, stats=s3)
    inf.generate(m, [p for p in prompts for _ in range(3)], 12, kv_page_size=64, graph=graph, stats=s1)
    assert len(tokens) == 9 and reasons == ["max_new_tokens"] * 9 and s3["n_samples"] == 3
    for p in range(3):
        assert tokens[3 * p] == tokens[3 * p + 1] == tokens[3 * p + 2] and len(tokens[3 * p]) == 12
    assert 0 < s3["kv_cache_bytes"] < s1["kv_cache_bytes"]
    if graph:
        assert s3["graph_replays"] > 0
