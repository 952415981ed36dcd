"""The regularised cross-entropy kernels (csrc/kernels/xent.hip: xent_fwd_reg / xent_reduce_reg / xent_bwd_reg)
against the fp64 oracle of tests/loss_reg_oracles.py, and the feature through the model, the captured step
and train.py on the GPU. Bounds as in tests/test_kernel_edges_gpu.py:

  16-bit storage: max|kernel - oracle| <= 2 * max|baseline - oracle| + 1 ulp at max|oracle|
  fp32 storage:   max|kernel - oracle| <= min(4 * measured, 2^-16) * max|oracle|

lse and the statistics are fp32 whatever the input dtype, so their rows cover all three input dtypes.
`measured` (FP32_MEASURED below) is the kernels' max|kernel - oracle| / max|oracle| over all cases of this
module, on an MI355X: the per-key maximum of `rel=` in the float32 lines of

  python -m pytest tests/test_loss_reg_gpu.py -s | grep ERR

  output          measured
  --------------  --------
  reg.lse         4.38e-08
  reg.objective   1.19e-07
  reg.nll         8.01e-08
  reg.zterm       1.94e-07
  reg.smooth      8.77e-08
  reg.lse_mean    7.37e-08
  reg.lse_absmax  4.38e-08
  reg.dlogits     3.31e-07

The inputs come from seeded CPU generators, so the figures repeat run to run.
"""
import math

import pytest
import torch

from pyrecover_amd import _ext
from pyrecover_amd.config import get_preset
from pyrecover_amd.models.llama import Transformer
from pyrecover_amd.ops import reference as R
from tests import loss_reg_oracles as L

pytestmark = pytest.mark.gpu

F32 = torch.float32
STAT_KEYS = ("objective", "nll", "zterm", "smooth", "lse_mean", "lse_absmax")
STAT_INDEX = {"objective": 0, "nll": 2, "zterm": 3, "smooth": 4, "lse_mean": 5, "lse_absmax": 6}
# the table above; the bound is 4x these, never above 2^-16 (kernel_oracles.fp32_bound)
FP32_MEASURED = {
    "reg.lse": 4.38e-08, "reg.objective": 1.19e-07, "reg.nll": 8.01e-08, "reg.zterm": 1.94e-07, "reg.smooth": 8.77e-08,
    "reg.lse_mean": 7.37e-08, "reg.lse_absmax": 4.38e-08, "reg.dlogits": 3.31e-07,
}
G = 0.5  # the upstream gradient of every kernel case


def _bound(key, base, oracle, storage):
    return L.fp32_bound(FP32_MEASURED[key], oracle) if storage == F32 else L.approx_bound(storage, base, oracle)


def _check(key, got, base, oracle, storage):
    """Print the figures, then assert the bound of the storage dtype."""
    e = L.err(got, oracle)
    mx = oracle.abs().max().item()
    bound = _bound(key, base, oracle, storage)
    print(f"ERR {key} {L.dname(storage)} err={e:.3e} rel={e / max(mx, 1e-300):.3e} base={L.err(base, oracle):.3e} "
          f"bound={bound:.3e}")
    assert torch.isfinite(got.double()).all(), key
    assert e <= bound, (key, e, bound)


def _run(C, buf, V, labels, g, z, eps):
    """Forward + in-place backward on a copy of the padded buffer: lse, stats (of the forward), dlogits."""
    work = buf.clone()
    lg = work[:, :V]
    lse, stats = C.xent_fwd_reg(lg, labels, L.IGNORE, z, eps)
    stats0 = stats.clone()
    C.xent_bwd_reg_(lg, labels, lse, stats, g, L.IGNORE, z, eps)
    assert torch.equal(work[:, V:], buf[:, V:])  # padding columns bit-unchanged
    return lse, stats0, lg


def _check_all(logits, lab, lse, stats, d, z, eps, dtype):
    lb, sb, db = L.reg_base(logits, lab, G, z, eps)
    lo, so, do = L.reg_oracle(logits, lab, G, z, eps)
    assert stats.shape == (8,) and stats.dtype == F32
    _check("reg.lse", lse, lb, lo, F32)
    assert stats[1].item() == so[1].item() and stats[7].item() == 0
    for k in STAT_KEYS:
        i = STAT_INDEX[k]
        _check("reg." + k, stats[i], sb[i], so[i], F32)
    _check("reg.dlogits", d, db, do, dtype)
    # objective = (1 - eps) nll + eps smooth + zterm, on the kernel's own entries (three fp32 roundings)
    want = (1 - eps) * stats[2].double() + eps * stats[4].double() + stats[3].double()
    assert abs(want.item() - stats[0].item()) <= 4 * 2.0 ** -24 * abs(want.item())
    return lo, so, db, do


# V = 8 (one chunk), 1001 and 2047 (< 2048: lanes that never load), 2049 (a tail of one), 50257 (many trips);
# label V - 1 lies in the scalar tail when V % 8 != 0; row 0 spreads over +-80, where 1 + 2 z lse is far from 1.
@pytest.mark.parametrize("T,V,ld", L.XENT_SHAPES)
@pytest.mark.parametrize("dtype", L.DTYPES, ids=L.dname)
@pytest.mark.parametrize("z,eps", L.COEFS)
def test_kernels_against_oracle(cuda, T, V, ld, dtype, z, eps):
    C = _ext.native()
    buf, logits, labels = L.xent_inputs(T, V, ld, dtype, cuda)
    g = torch.full((1,), G, device=cuda)
    for row0_ignored in (False, True):
        lab = labels.clone()
        if row0_ignored:
            lab[0] = L.IGNORE
        lse, stats, d = _run(C, buf, V, lab, g, z, eps)
        lo, so, db, do = _check_all(logits, lab, lse, stats, d, z, eps, dtype)
        ign = ~L.valid_rows(lab, V)
        if ign.any():
            assert d[ign].abs().max().item() == 0  # ignored rows exactly zero
        # each valid row of dlogits sums to 2 z lse g / n, within V times the dlogits bound
        want = 2 * z * lo * G / so[1] * (~ign).double()
        rs = (d.double().sum(-1) - want).abs().max().item()
        bound = V * _bound("reg.dlogits", db, do, dtype)
        print(f"ERR reg.rowsum {L.dname(dtype)} err={rs:.3e} bound={bound:.3e}")
        assert rs <= bound, (rs, bound)
        # two runs are bit-equal
        lse2, stats2, d2 = _run(C, buf, V, lab, g, z, eps)
        assert torch.equal(lse, lse2) and torch.equal(stats, stats2) and torch.equal(d, d2)


@pytest.mark.parametrize("T,V,ld", L.XENT_SHAPES)
@pytest.mark.parametrize("dtype", L.DTYPES, ids=L.dname)
def test_zero_coefficients_equal_the_plain_kernels_bitwise(cuda, T, V, ld, dtype):
    """z = 0, eps = 0: lse, the objective, n and dlogits are the plain kernels' on the same buffers, bit for
    bit (the factor is exactly 1.0f, the subtracted terms exactly the one-hot and 0)."""
    C = _ext.native()
    buf, logits, labels = L.xent_inputs(T, V, ld, dtype, cuda)
    g = torch.full((1,), G, device=cuda)
    lse, stats, d = _run(C, buf, V, labels, g, 0.0, 0.0)
    work = buf.clone()
    lg = work[:, :V]
    lse_p, _, stats_p = C.xent_fwd(lg, labels, L.IGNORE)
    C.xent_bwd_(lg, labels, lse_p, stats_p, g, L.IGNORE)
    assert torch.equal(lse, lse_p)
    assert torch.equal(stats[:2], stats_p)
    assert torch.equal(d, lg)
    assert stats[2].item() == stats[0].item() and stats[3].item() == 0 and stats[4].item() == 0


@pytest.mark.parametrize("T,V,ld", [(7, 1001, 1008), (4, 2049, 2056)])
@pytest.mark.parametrize("dtype", L.DTYPES, ids=L.dname)
def test_out_of_range_labels_are_ignored(cuda, T, V, ld, dtype):
    C = _ext.native()
    z, eps = L.COEFS[2]
    buf, logits, labels = L.xent_inputs(T, V, ld, dtype, cuda)
    g = torch.full((1,), G, device=cuda)
    bad, same = labels.clone(), labels.clone()
    bad[0], bad[1] = V, -7
    same[0] = same[1] = L.IGNORE
    lse, stats, d = _run(C, buf, V, bad, g, z, eps)
    lse2, stats2, d2 = _run(C, buf, V, same, g, z, eps)
    assert torch.equal(lse, lse2) and torch.equal(stats, stats2) and torch.equal(d, d2)
    assert stats[1].item() == T - 3 and d[:3].abs().max().item() == 0
    _check_all(logits, bad, lse, stats, d, z, eps, dtype)


@pytest.mark.parametrize("dtype", L.DTYPES, ids=L.dname)
@pytest.mark.parametrize("z,eps", L.COEFS)
def test_all_rows_ignored(cuda, dtype, z, eps):
    """No valid label: NaN objective (as the plain loss), n = 0, max |lse| = 0, all-zero dlogits."""
    C = _ext.native()
    T, V, ld = 4, 2049, 2056
    buf, logits, labels = L.xent_inputs(T, V, ld, dtype, cuda)
    labels.fill_(L.IGNORE)
    lse, stats, d = _run(C, buf, V, labels, torch.full((1,), G, device=cuda), z, eps)
    assert all(math.isnan(stats[i].item()) for i in (0, 2, 3, 4, 5))
    assert stats[1].item() == 0 and stats[6].item() == 0 and stats[7].item() == 0
    assert d.abs().max().item() == 0
    _check("reg.lse", lse, torch.logsumexp(R.up(logits), -1), torch.logsumexp(logits.double(), -1), F32)


@pytest.mark.parametrize("dtype", L.DTYPES, ids=L.dname)
@pytest.mark.parametrize("z,eps", L.COEFS)
def test_single_row(cuda, dtype, z, eps):
    """T = 1: the +-80 row alone (one block, a reduction over one row)."""
    C = _ext.native()
    V, ld = 2049, 2056
    buf, logits, labels = L.xent_inputs(4, V, ld, dtype, cuda)
    buf, logits, labels = buf[:1].clone(), None, labels[:1].clone()
    logits = buf[:, :V]
    lse, stats, d = _run(C, buf, V, labels, torch.full((1,), G, device=cuda), z, eps)
    assert stats[1].item() == 1
    _check_all(logits, labels, lse, stats, d, z, eps, dtype)


def test_rejections(cuda):
    C = _ext.native()
    logits = torch.randn(4, 1001, device=cuda, dtype=torch.bfloat16)
    labels = torch.zeros(4, dtype=torch.long, device=cuda)
    f = torch.zeros(12, device=cuda)
    lse, stats8, stats2, g = f[:4], f[4:12], f[4:6], torch.ones(1, device=cuda)
    with pytest.raises(RuntimeError, match=r"row stride % 8"):
        C.xent_fwd_reg(logits, labels, L.IGNORE, 1e-4, 0.1)
    with pytest.raises(RuntimeError, match=r"row stride % 8"):
        C.xent_bwd_reg_(logits, labels, lse, stats8, g, L.IGNORE, 1e-4, 0.1)
    ok = torch.randn(4, 1008, device=cuda, dtype=torch.bfloat16)[:, :1001]
    for z, eps in ((-1.0, 0.0), (float("nan"), 0.0), (float("inf"), 0.0), (0.0, 1.0), (0.0, -0.1), (0.0, float("nan"))):
        with pytest.raises(RuntimeError, match=r"z_loss|label_smoothing"):
            C.xent_fwd_reg(ok, labels, L.IGNORE, z, eps)
        with pytest.raises(RuntimeError, match=r"z_loss|label_smoothing"):
            C.xent_bwd_reg_(ok, labels, lse, stats8, g, L.IGNORE, z, eps)
    with pytest.raises(RuntimeError, match=r"stats"):
        C.xent_bwd_reg_(ok, labels, lse, stats2, g, L.IGNORE, 1e-4, 0.1)


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=L.dname)
def test_model_grads_vs_fp32_reference(cuda, dtype):
    """llama-micro with z = 1e-3, eps = 0.1: objective and gradients against the fp32 reference model, by the
    method and tolerances of tests/test_model_gpu.py::test_model_grads_vs_fp32_reference (16-bit: 5e-2)."""
    from tests.test_model_gpu import ref_forward

    z, eps = L.COEFS[2]
    torch.manual_seed(0)
    a = get_preset("llama-micro", seq_len=256)
    cpu = Transformer(a)
    B, S = 2, 256
    tok = torch.randint(0, a.vocab_size, (B, S))
    lab = torch.randint(0, a.vocab_size, (B, S))
    lab[:, :7] = -100
    loss_ref, stats_ref = R.cross_entropy_reg_ref(ref_forward(cpu, tok), lab, -100, z, eps)
    loss_ref.backward()
    gref = {n: p.grad.clone() for n, p in cpu.named_parameters()}

    gpu = Transformer(a)
    gpu.load_state_dict(cpu.state_dict())
    gpu = gpu.to(cuda, dtype)
    gpu.z_loss, gpu.label_smoothing = z, eps
    flat = gpu.flatten_()
    flat.zero_grad()
    loss = gpu(tok.to(cuda), labels=lab.to(cuda))
    loss.backward()
    tol = 5e-2
    assert abs(loss.item() - loss_ref.item()) < max(tol, 2e-3) * loss_ref.item()
    st = gpu.last_loss_stats
    assert st.is_cuda and st.shape == (8,) and st[0].item() == loss.item() and st[1].item() == stats_ref[1].item()
    for i in (2, 3, 4, 5, 6):
        assert abs(st[i].item() - stats_ref[i].item()) < max(tol, 2e-3) * abs(stats_ref[i].item()), i
    for n, p in gpu.named_parameters():
        assert p.grad.dtype == dtype
        g, r = p.grad.float().cpu(), gref[n]
        rel = ((g - r).norm() / r.norm().clamp_min(1e-12)).item()
        assert rel < tol, (n, rel)
    assert not any("loss" in k or "stats" in k for k in gpu.state_dict())


def _steps(cuda, graph: bool, steps=5):
    from pyrecover_amd.graph import StepGraph
    from pyrecover_amd.optim.adamw import FlatAdamW
    from pyrecover_amd.parallel.ddp import GradReducer

    torch.manual_seed(0)
    a = get_preset("llama-micro", seq_len=128)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    with torch.device(cuda):
        m = Transformer(a)
    torch.set_default_dtype(prev)
    m.z_loss, m.label_smoothing = L.COEFS[2]
    flat = m.flatten_()
    red = GradReducer(flat, bucket_cap_mb=0.5, first_bucket_mb=0.25)
    opt = FlatAdamW(flat, lr=1e-3)
    sg = StepGraph(m, opt, red) if graph else None
    gen = torch.Generator(device=cuda)
    gen.manual_seed(123)
    losses, stats = [], []
    for i in range(steps):
        t = torch.randint(0, a.vocab_size, (2, 129), device=cuda, generator=gen)
        x, y = t[:, :-1], t[:, 1:]
        if sg is not None and i >= 1:
            loss = sg.step(x, y)
            st = sg.stats
        else:
            opt.zero_grad()
            loss = m(x, labels=y)
            loss.backward()
            red.finish()
            opt.step()
            st = m.last_loss_stats
        losses.append(loss.detach().clone())
        stats.append(st.clone())
    torch.cuda.synchronize()
    return flat.data.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), torch.stack(losses), torch.stack(stats), sg


def test_graph_replay_equals_eager_bitwise(cuda):
    """The options are constants of the capture; every replay refreshes the static statistics tensor."""
    p0, m0, v0, l0, s0, _ = _steps(cuda, graph=False)
    p1, m1, v1, l1, s1, sg = _steps(cuda, graph=True)
    assert sg.captured and sg.replays == 4 and sg.stats is not None
    assert torch.equal(l0, l1) and torch.equal(s0, s1)
    assert torch.equal(s1[:, 0], l1) and len(set(s1[:, 0].tolist())) == 5  # refreshed by each replay
    assert torch.equal(p0, p1) and torch.equal(m0, m1) and torch.equal(v0, v1)


def _targs(ckdir, steps, extra=()):
    from pyrecover_amd.cli import get_args

    a = ["--model-preset", "llama-micro", "--synthetic-data", "--sequence-length", "128", "--batch-size", "2",
         "--training-steps", str(steps), "--checkpoint-dir", str(ckdir), "--experiment_name", "exp",
         "--checkpoint-frequency", "3", "--num-workers", "0", "--logging-frequency", "100",
         "--learning-rate", "1e-3", "--lr-warmup-steps", "2", "--compile", "--z-loss", "1e-4", "--label-smoothing", "0.1",
         "--loss-scale", "1"]
    return get_args(a + list(extra))


def _final(path):
    ck = torch.load(path, weights_only=True)
    return ck["model"], ck["optimizer"]["state"], ck["pyrecover_state"]


def test_train_compile_trains_and_resumes_bit_exact(cuda, tmp_path):
    """train.py --compile --z-loss 1e-4 --label-smoothing 0.1 --loss-scale 1: it trains, and a run stopped at
    step 4 and resumed ends bit-identical to the uninterrupted one; the returned loss is the plain
    cross-entropy."""
    from pyrecover_amd.trainer import train

    r = train(_targs(tmp_path / "straight", 6))
    assert r["step"] == 6 and math.isfinite(r["loss"]) and 0 < r["loss"] < 2 * math.log(get_preset("llama-micro").vocab_size)
    s = train(_targs(tmp_path / "split", 6, ["--stop-at-step", "4"]))
    assert s["stopped_early"] and s["step"] == 4
    train(_targs(tmp_path / "split", 6, ["--resume-from-checkpoint", "latest"]))
    a, b = _final(tmp_path / "straight" / "exp" / "ckpt_6.pt"), _final(tmp_path / "split" / "exp" / "ckpt_6.pt")
    for k in a[0]:
        assert torch.equal(a[0][k], b[0][k]), k
    for k in a[1]:
        for f in ("exp_avg", "exp_avg_sq", "step"):
            assert torch.equal(a[1][k][f], b[1][k][f]), (k, f)
    assert a[2]["loss"] == b[2]["loss"] == {"z_loss": 1e-4, "label_smoothing": 0.1}
