"""Document-masked attention (csrc/kernels/attention_docs.hip), packed RoPE and the packed training
step on the GPU, against the fp32 torch oracle (pyrecover_amd.ops.reference with doc_start).
Tolerances are those of tests/test_kernels_gpu.py and tests/test_model_gpu.py at these shapes."""
import math

import pytest
import torch

from pyrecover_amd import _ext
from pyrecover_amd.config import get_preset
from pyrecover_amd.models.llama import Transformer
from pyrecover_amd.ops import reference as R

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return ((a.float() - b.float()).abs().max() / b.float().abs().max().clamp_min(1e-6)).item()


def _qkv(cuda, B, S, Hq, Hkv, D, dtype=torch.bfloat16, seed=0):
    torch.manual_seed(seed)
    qkv = torch.randn(B * S, (Hq + 2 * Hkv) * D, device=cuda).to(dtype)
    q = qkv[:, :Hq * D].view(B, S, Hq, D)
    k = qkv[:, Hq * D:(Hq + Hkv) * D].view(B, S, Hkv, D)
    v = qkv[:, (Hq + Hkv) * D:].view(B, S, Hkv, D)
    return q, k, v


def _doc_start(rows, device):
    """int32 [B, S] from per-row document lengths."""
    out = []
    for lens in rows:
        r, p = [], 0
        for n in lens:
            r += [p] * n
            p += n
        out.append(r)
    return torch.tensor(out, dtype=torch.int32, device=device)


def _run(q, k, v, do, ds, scale):
    C = _ext.native()
    o, lse = C.attn_fwd(q, k, v, scale, True, ds)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    C.attn_bwd(q, k, v, o, do, lse, dq, dk, dv, scale, True, None, 0, ds)
    return o, lse, dq, dk, dv


def _oracle(q, k, v, do, ds, scale):
    qf, kf, vf = (t.float().requires_grad_() for t in (q, k, v))
    of, lf = R.attention_lse_ref(qf, kf, vf, True, scale, doc_start=ds)
    of.backward(do.float())
    return of.detach(), lf.detach(), qf.grad, kf.grad, vf.grad


def _check(got, want):
    o, lse, dq, dk, dv = got
    of, lf, gq, gk, gv = want
    print("max|o - o_ref|", (o.float() - of).abs().max().item(), "max|lse - lse_ref|", (lse - lf).abs().max().item(),
          "rel dq dk dv", _rel(dq, gq), _rel(dk, gk), _rel(dv, gv))
    assert (o.float() - of).abs().max().item() < 2e-2
    assert (lse - lf).abs().max().item() < 1e-3
    for g, w in ((dq, gq), (dk, gk), (dv, gv)):
        assert _rel(g, w) < 3e-2, _rel(g, w)


LAYOUTS = {
    # a 1-token document; boundaries inside a 32-row wave tile, on its edge and on the 64-key tile edge
    "mixed256": (1, 256, [[1, 31, 32, 33, 63, 64, 32]]),
    # per-row indexing; multi-tile documents with an unaligned boundary
    "rows1024": (2, 1024, [[1024], [300, 724]]),
    # S % 128 != 0: the zero-padding path
    "pad200": (1, 200, [[100, 100]]),
    # one document: plain causal attention
    "single256": (1, 256, [[256]]),
}


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("Hq,Hkv", [(4, 4), (8, 2)])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_docs_attention_matches_oracle(cuda, dtype, D, Hq, Hkv, layout):
    B, S, rows = LAYOUTS[layout]
    q, k, v = _qkv(cuda, B, S, Hq, Hkv, D, dtype)
    do = torch.randn(B, S, Hq, D, device=cuda).to(dtype)
    ds = _doc_start(rows, cuda)
    scale = 1 / math.sqrt(D)
    got = _run(q, k, v, do, ds, scale)
    _check(got, _oracle(q, k, v, do, ds, scale))
    again = _run(q, k, v, do, ds, scale)
    assert all(torch.equal(a, b) for a, b in zip(got, again))  # bit-reproducible, forward and backward
    if layout == "single256":  # doc_start all zeros agrees with the plain causal kernels
        C = _ext.native()
        o, lse = C.attn_fwd(q, k, v, scale, True)
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        C.attn_bwd(q, k, v, o, do, lse, dq, dk, dv, scale, True)
        _check(got, (o.float(), lse, dq.float(), dk.float(), dv.float()))


@pytest.mark.parametrize("D,Hq,Hkv", [(128, 4, 4), (64, 8, 2)])
def test_docs_attention_skips_invisible_tiles(cuda, D, Hq, Hkv):
    """Tiles no query of a block can see are never touched: +inf planted there (which 0 * inf would
    turn into NaN) leaves the other document's results equal to that document run alone."""
    B, S, H = 1, 1024, 512
    q, k, v = _qkv(cuda, B, S, Hq, Hkv, D, seed=3)
    do = torch.randn(B, S, Hq, D, device=cuda).bfloat16()
    ds = _doc_start([[H, H]], cuda)
    scale = 1 / math.sqrt(D)
    zeros = torch.zeros(B, H, dtype=torch.int32, device=cuda)
    # V of the first document = +inf: O and dQ of the second document
    vi = v.clone()
    vi[:, :H] = float("inf")
    o, lse, dq, _, _ = _run(q, k, vi, do, ds, scale)
    of, lf, gq, _, _ = _oracle(q[:, H:], k[:, H:], v[:, H:], do[:, H:], zeros, scale)
    assert (o[:, H:].float() - of).abs().max().item() < 2e-2
    assert (lse[:, :, H:] - lf).abs().max().item() < 1e-3
    assert _rel(dq[:, H:], gq) < 3e-2
    # dO of the second document = +inf: dK and dV of the first document
    doi = do.clone()
    doi[:, H:] = float("inf")
    _, _, _, dk, dv = _run(q, k, v, doi, ds, scale)
    _, _, _, gk, gv = _oracle(q[:, :H], k[:, :H], v[:, :H], do[:, :H], zeros, scale)
    assert _rel(dk[:, :H], gk) < 3e-2 and _rel(dv[:, :H], gv) < 3e-2


def test_docs_attention_clamps_garbage_doc_start(cuda):
    """Negative values, values above i and decreasing runs: every value is clamped into [0, i]
    (pyrecover_amd.ops.reference.doc_mask clamps the same way), so each row keeps at least its own
    key, the result is finite and equals the oracle of the clamped mask. (That no access leaves the
    row follows from the index math: key tiles run from clamp(doc_start) / 64 >= 0 to the block's
    diagonal, query tiles from the key block to a bound clamped to S.)"""
    B, S, Hq, Hkv, D = 2, 384, 4, 2, 128
    q, k, v = _qkv(cuda, B, S, Hq, Hkv, D, seed=5)
    do = torch.randn(B, S, Hq, D, device=cuda).bfloat16()
    g = torch.Generator().manual_seed(0)
    ds = torch.randint(-1000, 2000, (B, S), generator=g, dtype=torch.int32)
    ds[0, 100:200] = torch.arange(199, 99, -1, dtype=torch.int32)  # a decreasing run
    ds[1, :64] = -(2 ** 31)
    ds[1, 64:128] = 2 ** 31 - 1
    ds = ds.to(cuda)
    scale = 1 / math.sqrt(D)
    got = _run(q, k, v, do, ds, scale)
    assert all(torch.isfinite(t.float()).all() for t in got)
    _check(got, _oracle(q, k, v, do, ds, scale))


def test_flash_attention_with_doc_start(cuda):
    """The public op: pyrecover_amd.ops.flash_attention(..., doc_start=) with autograd (any integer
    dtype of doc_start), GQA, against the oracle."""
    from pyrecover_amd.ops import flash_attention

    B, S, Hq, Hkv, D = 2, 256, 8, 2, 64
    q, k, v = (t.clone().requires_grad_() for t in _qkv(cuda, B, S, Hq, Hkv, D, seed=2))
    do = torch.randn(B, S, Hq, D, device=cuda).bfloat16()
    ds = _doc_start([LAYOUTS["mixed256"][2][0], [100, 156]], cuda)
    o = flash_attention(q, k, v, doc_start=ds.long())
    o.backward(do)
    of, _, gq, gk, gv = _oracle(q.detach(), k.detach(), v.detach(), do, ds, 1 / math.sqrt(D))
    assert (o.float() - of).abs().max().item() < 2e-2
    for g, w in ((q.grad, gq), (k.grad, gk), (v.grad, gv)):
        assert _rel(g, w) < 3e-2, _rel(g, w)
    with pytest.raises(ValueError):
        flash_attention(q, k, v, causal=False, doc_start=ds)


def test_docs_binding_rejects_bad_doc_start(cuda):
    C = _ext.native()
    q, k, v = _qkv(cuda, 1, 128, 2, 2, 64)
    scale = 0.125
    with pytest.raises(RuntimeError):
        C.attn_fwd(q, k, v, scale, True, torch.zeros(1, 128, dtype=torch.int64, device=cuda))
    with pytest.raises(RuntimeError):
        C.attn_fwd(q, k, v, scale, True, torch.zeros(1, 64, dtype=torch.int32, device=cuda))
    with pytest.raises(RuntimeError):
        C.attn_fwd(q, k, v, scale, True, torch.zeros(1, 128, dtype=torch.int32))
    with pytest.raises(RuntimeError):
        C.attn_fwd(q, k, v, scale, False, torch.zeros(1, 128, dtype=torch.int32, device=cuda))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_rope_with_doc_start(cuda, dtype):
    C = _ext.native()
    B, S, Hq, Hkv, D = 2, 256, 4, 2, 128
    tab = R.rope_table(R.precompute_freqs_cis(D, S, 500000.0)).to(cuda)
    torch.manual_seed(0)
    qkv = torch.randn(B * S, (Hq + 2 * Hkv) * D, device=cuda).to(dtype)
    ds = _doc_start([LAYOUTS["mixed256"][2][0], [100, 156]], cuda)
    n = (Hq + Hkv) * D
    x, want = qkv.clone(), qkv.clone()
    C.rope_(x, n, tab, D, S, 0, False, ds)
    R.rope_inplace_2d(want, n, tab, D, S, doc_start=ds)
    assert _rel(x, want) < 1e-2
    assert torch.equal(x[:, n:], qkv[:, n:])
    plain = qkv.clone()
    C.rope_(plain, n, tab, D, S, 0, False)
    assert torch.equal(plain[:1], x[:1]) and not torch.equal(plain[1:S], x[1:S])  # positions restart
    C.rope_(x, n, tab, D, S, 0, True, ds)  # the inverse rotation restores
    R.rope_inplace_2d(want, n, tab, D, S, inverse=True, doc_start=ds)
    assert _rel(x, qkv) < 2e-2 and _rel(x, want) < 2e-2


# ------------------------------------------------------------------------------------------
def test_packed_model_grads_vs_fp32_cpu_oracle(cuda):
    """bf16 llama-micro, forward and backward with packing on the HIP kernels, against the fp32 CPU
    torch path; bounds of tests/test_model_gpu.py::test_model_grads_vs_fp32_reference (bf16, B2 S256)."""
    torch.manual_seed(0)
    a = get_preset("llama-micro", seq_len=256)
    cpu = Transformer(a)
    B, S = 2, 256
    tok = torch.randint(0, a.vocab_size, (B, S))
    lab = torch.randint(0, a.vocab_size, (B, S))
    lab[:, :7] = -100
    ds = _doc_start([LAYOUTS["mixed256"][2][0], [100, 156]], "cpu")
    loss_ref = cpu(tok, labels=lab, doc_start=ds)
    loss_ref.backward()
    gref = {n: p.grad.clone() for n, p in cpu.named_parameters()}
    unpacked = cpu(tok, labels=lab).item()
    assert abs(unpacked - loss_ref.item()) > 1e-4  # the mask is in effect

    gpu = Transformer(a)
    gpu.load_state_dict(cpu.state_dict())
    gpu = gpu.to(cuda, torch.bfloat16)
    flat = gpu.flatten_()
    flat.zero_grad()
    loss = gpu(tok.to(cuda), labels=lab.to(cuda), doc_start=ds.to(cuda))
    loss.backward()
    tol = 5e-2
    assert abs(loss.item() - loss_ref.item()) < tol * loss_ref.item()
    for n, p in gpu.named_parameters():
        g, r = p.grad.float().cpu(), gref[n]
        rel = ((g - r).norm() / r.norm().clamp_min(1e-12)).item()
        assert rel < tol, (n, rel)


def _packed_steps(cuda, graph: bool, overlap: bool, steps: int, recompute: bool = False):
    from pyrecover_amd.graph import StepGraph
    from pyrecover_amd.optim.adamw import FlatAdamW
    from pyrecover_amd.optim.lr import build_lr_scheduler
    from pyrecover_amd.parallel.ddp import GradReducer

    torch.manual_seed(0)
    a = get_preset("llama-tiny", seq_len=256)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    with torch.device(cuda):
        m = Transformer(a)
    torch.set_default_dtype(prev)
    m.activation_checkpointing = recompute
    flat = m.flatten_()
    red = GradReducer(flat, bucket_cap_mb=0.5, first_bucket_mb=0.25)
    opt = FlatAdamW(flat, lr=1e-3)
    if overlap:
        opt.enable_overlap(red)
    sched = build_lr_scheduler(opt, 3)
    sg = StepGraph(m, opt, red) if graph else None
    gen = torch.Generator(device=cuda)
    gen.manual_seed(123)
    layouts = [[[1, 31, 32, 33, 63, 64, 32], [100, 156]], [[256], [7, 249]], [[128, 128], [64, 64, 64, 64]]]
    losses = []
    for i in range(steps):
        t = torch.randint(0, a.vocab_size, (2, 257), device=cuda, generator=gen)
        x, y, ds = t[:, :-1], t[:, 1:], _doc_start(layouts[i % 3], cuda)
        if sg is not None and i >= 2:
            loss = sg.step(x, y, ds)
        else:
            opt.zero_grad()
            loss = m(x, labels=y, doc_start=ds)
            loss.backward()
            red.finish()
            opt.step()
        sched.step()
        losses.append(loss.detach().float().item())
    torch.cuda.synchronize()
    return flat.data.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), losses, sg


def test_packed_graph_step_matches_eager(cuda):
    """The packed step under --compile (hipGraph replay, doc_start copied into a static buffer per
    step) is bitwise equal to the eager step, as tests/test_graph_gpu.py asserts for the unpacked one."""
    p0, m0, v0, l0, _ = _packed_steps(cuda, graph=False, overlap=True, steps=6)
    p1, m1, v1, l1, sg = _packed_steps(cuda, graph=True, overlap=True, steps=6)
    assert sg.captured and sg.replays == 4
    assert l0 == l1
    assert torch.equal(p0, p1) and torch.equal(m0, m1) and torch.equal(v0, v1)


def test_packed_overlapped_optimizer_is_bit_identical(cuda):
    """4 packed steps with the AdamW update overlapped (enqueued behind the event the attention
    backward records between its dQ and dK/dV kernels) and 4 with the plain update: same bits."""
    from pyrecover_amd.ops import sched

    p0, m0, v0, l0, _ = _packed_steps(cuda, graph=False, overlap=False, steps=4)
    w0 = sched.windows_fired()
    p1, m1, v1, l1, _ = _packed_steps(cuda, graph=False, overlap=True, steps=4)
    assert sched.windows_fired() > w0  # the packed backward offers the window
    assert l0 == l1 and torch.equal(p0, p1) and torch.equal(m0, m1) and torch.equal(v0, v1)
    p2, _, v2, _, _ = _packed_steps(cuda, graph=False, overlap=True, steps=4, recompute=True)
    assert torch.equal(p0, p2) and torch.equal(v0, v2)  # activation checkpointing passes doc_start on


def test_train_py_pack_sequences_compile(cuda, tmp_path):
    """train.py --pack-sequences --compile on the GPU: same final checkpoint as the eager run."""
    from pyrecover_amd.cli import get_args
    from pyrecover_amd.trainer import train

    def run(name, extra):
        train(get_args(["--model-preset", "llama-tiny", "--synthetic-data", "--sequence-length", "256",
                        "--batch-size", "2", "--training-steps", "5", "--checkpoint-dir", str(tmp_path / name),
                        "--experiment_name", "exp", "--checkpoint-frequency", "5", "--num-workers", "0",
                        "--logging-frequency", "100", "--learning-rate", "1e-3", "--lr-warmup-steps", "2",
                        "--pack-sequences"] + extra))
        ck = torch.load(tmp_path / name / "exp" / "ckpt_5.pt", weights_only=True)
        return ck["model"], ck["optimizer"]["state"]

    a, b = run("eager", []), run("graph", ["--compile"])
    for k in a[0]:
        assert torch.equal(a[0][k], b[0][k]), k
    for k in a[1]:
        assert torch.equal(a[1][k]["exp_avg_sq"], b[1][k]["exp_avg_sq"]), k
