"""--z-loss, --label-smoothing and --logit-stats on the CPU: the fp64 oracle of tests/loss_reg_oracles.py
against torch, the project's reference against the oracle, the ops and the model, and train.py (JSONL fields,
what "loss" means, checkpoint key, bit-exact resume, accumulation, flag validation). The HIP kernels are
tested against the same oracle in tests/test_loss_reg_gpu.py."""
import json
import logging
import math

import pytest
import torch

from pyrecover_amd.ops import fused as FU
from pyrecover_amd.ops import reference as R
from tests import loss_reg_oracles as L
from tests.test_distributed import _argv, _run

CPU = torch.device("cpu")
F32 = torch.float32


def _labels(labels, row0_ignored):
    lab = labels.clone()
    if row0_ignored:
        lab[0] = L.IGNORE
    return lab


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,V,ld", L.XENT_SHAPES)
@pytest.mark.parametrize("z,eps", L.COEFS)
@pytest.mark.parametrize("row0_ignored", [False, True])
def test_oracle_equals_torch_autograd(T, V, ld, z, eps, row0_ignored):
    """The closed forms equal F.cross_entropy(label_smoothing=) + the z term and their autograd gradient in
    fp64: 1e-12 relative on the objective, 1e-12 absolute on dlogits."""
    _, logits, labels = L.xent_inputs(T, V, ld, torch.float64, CPU)
    lab = _labels(labels, row0_ignored)
    x = logits.clone().requires_grad_()
    obj = L.torch_objective(x, lab, z, eps)
    obj.backward()
    lse, stats, d = L.reg_oracle(logits, lab, 0.5, z, eps)
    assert abs(stats[0].item() - obj.item()) <= 1e-12 * abs(obj.item())
    assert (d - 0.5 * x.grad).abs().max().item() <= 1e-12
    assert stats[1].item() == lab.ne(L.IGNORE).sum().item()
    # the identity between the entries, with the smoothing term formed from the rows
    sm = ((lse - logits.mean(-1)) * lab.ne(L.IGNORE)).sum() / stats[1]
    assert abs(((1 - eps) * stats[2] + eps * sm + stats[3] - stats[0]).item()) <= 1e-12 * abs(obj.item())


@pytest.mark.parametrize("T,V,ld", L.XENT_SHAPES)
@pytest.mark.parametrize("dtype", L.DTYPES, ids=L.dname)
@pytest.mark.parametrize("z,eps", L.COEFS)
def test_baseline_within_caps(T, V, ld, dtype, z, eps):
    """cross_entropy_reg_ref + autograd against the oracle: fp32 outputs under the 2^-16 cap (a condition),
    16-bit dlogits within one storage ulp (fp32 math and one rounding differ from the rounded oracle only at a
    tie), so the GPU test's 2 * err(baseline) + 1 ulp amounts to about one ulp."""
    _, logits, labels = L.xent_inputs(T, V, ld, dtype, CPU)
    for row0_ignored in (False, True):
        lab = _labels(labels, row0_ignored)
        lb, sb, db = L.reg_base(logits, lab, 0.5, z, eps)
        lo, so, do = L.reg_oracle(logits, lab, 0.5, z, eps)
        assert L.err(lb, lo) <= L.fp32_bound(1.0, lo)
        for i, name in enumerate(L.STAT_NAMES):
            assert abs(sb[i].item() - so[i].item()) <= L.fp32_bound(1.0, so[i]), name
        mx = do.abs().max().item()
        e = L.err(db, do)
        if dtype == F32:
            assert e <= L.fp32_bound(1.0, do)
        else:
            assert e <= L.ulp_at(dtype, mx), (e, mx)
        assert L.approx_bound(dtype, db, do) >= e


@pytest.mark.parametrize("T,V,ld", L.XENT_SHAPES)
@pytest.mark.parametrize("z,eps", L.COEFS)
def test_oracle_row_sums(T, V, ld, z, eps):
    """Each valid row of dlogits sums to 2 z lse g / n (0 for the plain loss), an ignored row to 0."""
    _, logits, labels = L.xent_inputs(T, V, ld, torch.float64, CPU)
    g = 0.5
    lse, stats, d = L.reg_oracle(logits, labels, g, z, eps)
    valid = L.valid_rows(labels, V).double()
    want = 2 * z * lse * g / stats[1] * valid
    assert (d.sum(-1) - want).abs().max().item() <= 1e-12


def test_reference_defaults_equal_plain_loss():
    _, logits, labels = L.xent_inputs(7, 1001, 1008, F32, CPU)
    obj, stats = R.cross_entropy_reg_ref(logits, labels, L.IGNORE)
    plain = R.cross_entropy_ref(logits, labels, L.IGNORE)
    assert abs(obj.item() - plain.item()) <= 1e-6 * plain.item()
    assert stats.shape == (8,) and stats[3].item() == 0 and stats[4].item() == 0 and stats[7].item() == 0
    none = torch.full_like(labels, L.IGNORE)
    obj, stats = R.cross_entropy_reg_ref(logits, none, L.IGNORE, 1e-3, 0.1)
    assert math.isnan(obj.item()) and stats[1].item() == 0 and stats[6].item() == 0
    assert all(math.isnan(stats[i].item()) for i in (0, 2, 3, 4, 5))


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("z,eps", L.COEFS)
def test_linear_cross_entropy_cpu_grads(z, eps):
    """The op's CPU branch (closed-form backward): dh and dW against fp64 autograd of the written-out formula."""
    T, D, V = 6, 16, 40
    g = torch.Generator().manual_seed(1)
    h = torch.randn(T, D, generator=g, dtype=torch.float64)
    W = torch.randn(V, D, generator=g, dtype=torch.float64)
    lab = torch.randint(0, V, (T,), generator=g)
    lab[2] = -100
    hh, WW = h.clone().requires_grad_(), W.clone().requires_grad_()
    x = hh @ WW.t()
    lse = torch.logsumexp(x, -1)
    valid = lab.ne(-100)
    n = valid.sum()
    nll = lse - x.gather(1, lab.clamp_min(0)[:, None])[:, 0]
    want = (((1 - eps) * nll + eps * (lse - x.mean(-1)) + z * lse ** 2) * valid).sum() / n
    (3.0 * want).backward()

    h1 = h.clone().requires_grad_()
    Wp = torch.nn.Parameter(W.clone())
    loss, stats = FU.linear_cross_entropy_stats(h1, Wp.detach(), lab, FU.UnflatSlot([Wp]), Wp, z_loss=z,
                                                label_smoothing=eps)
    (3.0 * loss).backward()
    assert abs(loss.item() - want.item()) <= 1e-12 * abs(want.item())
    assert (h1.grad - hh.grad).abs().max().item() <= 1e-12
    assert (Wp.grad - WW.grad).abs().max().item() <= 1e-12
    assert not stats.requires_grad and stats[0].item() == loss.item() and stats[1].item() == T - 1
    # the objective-only entry point returns the same value
    again = FU.linear_cross_entropy(h.clone(), Wp.detach(), lab, FU.UnflatSlot([Wp]), Wp, z_loss=z, label_smoothing=eps)
    assert again.item() == loss.item()


def test_linear_cross_entropy_rejects_bad_coefficients():
    h, W = torch.randn(2, 4), torch.nn.Parameter(torch.randn(8, 4))
    lab = torch.tensor([1, 2])
    for kw in ({"z_loss": -1.0}, {"z_loss": float("nan")}, {"z_loss": float("inf")}, {"label_smoothing": 1.0},
               {"label_smoothing": -0.1}):
        with pytest.raises(ValueError):
            FU.linear_cross_entropy(h, W.detach(), lab, FU.UnflatSlot([W]), W, **kw)


# ------------------------------------------------------------------------------------------------
def _micro(seed=0):
    from pyrecover_amd.config import get_preset
    from pyrecover_amd.models.llama import Transformer

    torch.manual_seed(seed)
    cfg = get_preset("llama-micro", seq_len=32)
    m = Transformer(cfg)
    x = torch.randint(0, cfg.vocab_size, (2, 33), generator=torch.Generator().manual_seed(3))
    return m, x[:, :-1], x[:, 1:].clone()


def test_model_options_off_is_bitwise_the_plain_model(monkeypatch):
    """With every option at its default the Transformer never reaches the regularised head: loss and
    gradients are bit-equal to a model on which that head does not exist, and the options are not state."""
    a, x, y = _micro()
    b, _, _ = _micro()
    assert a.z_loss == 0.0 and a.label_smoothing == 0.0 and a.logit_stats is False and not a.loss_regularised
    assert not any("loss" in k or "smooth" in k or "stats" in k for k in a.state_dict())
    la = a(x, labels=y)
    la.backward()

    def gone(*args, **kw):
        raise AssertionError("the regularised head ran with the options off")

    monkeypatch.setattr(FU, "linear_cross_entropy_stats", gone)
    monkeypatch.setattr(FU._LinearCrossEntropyReg, "apply", gone)
    lb = b(x, labels=y)
    lb.backward()
    assert torch.equal(la, lb) and a.last_loss_stats is None
    for (k, p), q in zip(a.named_parameters(), b.parameters()):
        assert torch.equal(p.grad, q.grad), k


def test_model_stats_and_logit_stats_alone():
    a, x, y = _micro()
    b, _, _ = _micro()
    lp = a(x, labels=y)
    lp.backward()
    b.logit_stats = True
    ls = b(x, labels=y)
    ls.backward()
    st = b.last_loss_stats
    assert st.shape == (8,) and not st.requires_grad
    assert abs(ls.item() - lp.item()) <= 1e-6 * lp.item() and st[2].item() == st[0].item()
    assert st[5].item() > 0 and st[6].item() >= st[5].item()
    for (k, p), q in zip(a.named_parameters(), b.parameters()):
        assert torch.allclose(p.grad, q.grad, rtol=1e-5, atol=1e-7), k
    b.logit_stats, b.z_loss, b.label_smoothing = False, 1e-3, 0.1
    lo = b(x, labels=y)
    st = b.last_loss_stats
    assert lo.item() == st[0].item() and lo.item() > st[2].item()
    want = 0.9 * st[2] + 0.1 * st[4] + st[3]
    assert abs(want.item() - lo.item()) <= 1e-6 * lo.item()


# ------------------------------------------------------------------------------------------------
# train.py, llama-micro on the CPU
STEPS = 6
REG = ["--z-loss", "1e-4", "--label-smoothing", "0.1"]


def _ckpt(path):
    return torch.load(path, weights_only=True)


def _same_state(a, b, equal=True):
    diff = 0
    for k in a["model"]:
        diff += int(not torch.equal(a["model"][k], b["model"][k]))
    for i, st in a["optimizer"]["state"].items():
        for k in ("exp_avg", "exp_avg_sq"):
            diff += int(not torch.equal(st[k], b["optimizer"]["state"][i][k]))
    assert (diff == 0) if equal else (diff > 0), diff


def _jsonl(path):
    return [json.loads(line) for line in open(path)]


NEW_FIELDS = ("objective", "z_loss_term", "smoothing_term", "lse_mean", "lse_absmax")


@pytest.fixture(scope="module")
def straight(tmp_path_factory):
    """The uninterrupted 6-step regularised run, logging every step."""
    tmp = tmp_path_factory.mktemp("lr")
    res = _run(1, _argv(tmp / "s", STEPS, REG + ["--metrics-jsonl", str(tmp / "s.jsonl"), "--logging-frequency", "1"]),
               tmp)
    return tmp, res


def test_train_jsonl_fields_and_loss_meaning(straight):
    tmp, res = straight
    recs = _jsonl(tmp / "s.jsonl")
    assert [r["step"] for r in recs] == list(range(1, STEPS + 1))
    for r in recs:
        assert all(k in r for k in NEW_FIELDS)
        tot = r["loss"] + r["smoothing_term"] + r["z_loss_term"]
        assert abs(r["objective"] - tot) <= 4 * 2.0 ** -24 * abs(r["objective"])  # fp32 rounding of three terms
        assert r["objective"] != r["loss"] and r["z_loss_term"] > 0 and r["smoothing_term"] != 0
        assert 0 < r["lse_mean"] <= r["lse_absmax"]
    # "loss" is the plain cross-entropy: the returned summary's too
    assert res["loss"] == recs[-1]["loss"]
    # an untrained llama-micro starts near log(V) in the plain loss
    from pyrecover_amd.config import get_preset

    assert abs(recs[0]["loss"] - math.log(get_preset("llama-micro").vocab_size)) < 1.0


def test_checkpoint_records_the_objective(straight, tmp_path):
    tmp, _ = straight
    ck = _ckpt(tmp / "s" / "e" / f"ckpt_{STEPS}.pt")
    assert ck["pyrecover_state"]["loss"] == {"z_loss": 1e-4, "label_smoothing": 0.1}
    assert not any("loss" in k or "stats" in k for k in ck["model"])
    _run(1, _argv(tmp_path / "o", 1, ["--checkpoint-frequency", "1"]), tmp_path)
    assert "loss" not in _ckpt(tmp_path / "o" / "e" / "ckpt_1.pt")["pyrecover_state"]


@pytest.mark.parametrize("fmt", ["vanilla", "sharded"])
def test_resume_is_bitwise(straight, tmp_path, fmt):
    tmp, _ = straight
    f = ["--use-torch-distributed-ckpt"] if fmt == "sharded" else []
    _run(1, _argv(tmp_path / "r", STEPS, REG + f + ["--stop-at-step", "3"]), tmp_path)
    _run(1, _argv(tmp_path / "r", STEPS, REG + f + ["--resume-from-checkpoint", "latest"]), tmp_path)
    ref = _ckpt(tmp / "s" / "e" / f"ckpt_{STEPS}.pt")
    if fmt == "vanilla":
        got = _ckpt(tmp_path / "r" / "e" / f"ckpt_{STEPS}.pt")
    else:
        from pyrecover_amd.ckpt.sharded import build_ckpt, read_sharded_state

        got = build_ckpt(read_sharded_state(str(tmp_path / "r" / "e" / f"ckpt_{STEPS}")))
    _same_state(ref, got)
    rec = got["pyrecover_state"]["loss"]
    assert {k: float(v) for k, v in rec.items()} == {"z_loss": 1e-4, "label_smoothing": 0.1}


def test_resume_under_another_z_loss_warns_and_uses_the_flag(straight, tmp_path, caplog):
    tmp, _ = straight
    _run(1, _argv(tmp_path / "m", STEPS, REG + ["--stop-at-step", "3"]), tmp_path)
    with caplog.at_level(logging.WARNING, logger="pyrecover"):
        _run(1, _argv(tmp_path / "m", STEPS, ["--z-loss", "1e-2", "--label-smoothing", "0.1",
                                              "--resume-from-checkpoint", "latest"]), tmp_path)
    assert any("--z-loss 0.01 (checkpoint: 0.0001)" in r.getMessage() for r in caplog.records)
    ck = _ckpt(tmp_path / "m" / "e" / f"ckpt_{STEPS}.pt")
    assert ck["pyrecover_state"]["loss"] == {"z_loss": 1e-2, "label_smoothing": 0.1}
    _same_state(_ckpt(tmp / "s" / "e" / f"ckpt_{STEPS}.pt"), ck, equal=False)
    # the same flags: no warning
    caplog.clear()
    with caplog.at_level(logging.WARNING, logger="pyrecover"):
        _run(1, _argv(tmp_path / "m", STEPS + 1, ["--z-loss", "1e-2", "--label-smoothing", "0.1",
                                                  "--resume-from-checkpoint", "latest"]), tmp_path)
    assert not any("objective" in r.getMessage() for r in caplog.records)


def test_logit_stats_alone_trains_like_a_plain_run(tmp_path):
    """--logit-stats with both coefficients zero: the parameters after 5 steps are bit-equal to a plain run's
    (on the CPU both heads run the same torch math for the gradient), and lse_mean is logged."""
    ex = ["--checkpoint-frequency", "5", "--logging-frequency", "1"]
    _run(1, _argv(tmp_path / "p", 5, ex + ["--metrics-jsonl", str(tmp_path / "p.jsonl")]), tmp_path)
    _run(1, _argv(tmp_path / "t", 5, ex + ["--logit-stats", "--metrics-jsonl", str(tmp_path / "t.jsonl")]), tmp_path)
    _same_state(_ckpt(tmp_path / "p" / "e" / "ckpt_5.pt"), _ckpt(tmp_path / "t" / "e" / "ckpt_5.pt"))
    plain, tele = _jsonl(tmp_path / "p.jsonl"), _jsonl(tmp_path / "t.jsonl")
    assert "lse_mean" not in plain[0] and "objective" not in plain[0]
    for p, t in zip(plain, tele):
        assert t["lse_mean"] > 0 and t["z_loss_term"] == 0 and t["smoothing_term"] == 0
        assert abs(t["loss"] - p["loss"]) <= 1e-6 * p["loss"] and t["objective"] == t["loss"]


def test_accumulation_averages_the_statistics(tmp_path):
    """--grad-accumulation-steps 2 at batch 2 sees the samples of one batch-4 step... not the same batches, so
    the check is on the model: the logged statistics of step 1 equal the mean (lse_absmax: the maximum) of the
    two micro-batches' statistics, recomputed from the run's own initial model and data."""
    from pyrecover_amd.cli import get_args
    from pyrecover_amd import trainer as TR

    seen = []
    orig = TR.Transformer.forward

    def spy(self, *a, **kw):
        out = orig(self, *a, **kw)
        if self.last_loss_stats is not None:
            seen.append(self.last_loss_stats.clone())
        return out

    argv = _argv(tmp_path / "a", 2, REG + ["--grad-accumulation-steps", "2", "--batch-size", "2", "--logging-frequency",
                                          "1", "--metrics-jsonl", str(tmp_path / "a.jsonl")])
    TR.Transformer.forward = spy
    try:
        TR.train(get_args(argv))
    finally:
        TR.Transformer.forward = orig
    recs = _jsonl(tmp_path / "a.jsonl")
    assert len(seen) == 4 and len(recs) == 2
    for r, (s0, s1) in zip(recs, ((seen[0], seen[1]), (seen[2], seen[3]))):
        mean = (s0 + s1) / 2
        assert r["loss"] == pytest.approx(mean[2].item(), rel=1e-6)
        assert r["objective"] == pytest.approx(mean[0].item(), rel=1e-6)
        assert r["z_loss_term"] == pytest.approx(mean[3].item(), rel=1e-6)
        assert r["lse_mean"] == pytest.approx(mean[5].item(), rel=1e-6)
        assert r["lse_absmax"] == max(s0[6].item(), s1[6].item())
        assert r["smoothing_term"] == pytest.approx(0.1 * (mean[4] - mean[2]).item(), rel=1e-5)


def test_cli_validation():
    from pyrecover_amd.cli import get_args

    a = get_args([])
    assert a.z_loss == 0.0 and a.label_smoothing == 0.0 and a.logit_stats is False
    a = get_args(["--z-loss", "1e-4", "--label-smoothing", "0.1", "--logit-stats"])
    assert a.z_loss == 1e-4 and a.label_smoothing == 0.1 and a.logit_stats is True
    for bad in (["--z-loss", "-1"], ["--label-smoothing", "1"], ["--z-loss", "nan"], ["--label-smoothing", "nan"],
                ["--z-loss", "inf"], ["--label-smoothing", "-0.5"]):
        with pytest.raises(SystemExit):
            get_args(bad)
