"""--loss-scale: the scale state machine, the skipped update and the non-finite guard end to end, on
the CPU (the rule the HIP guard kernel implements runs in Python there; tests/test_loss_scale_gpu.py
checks the kernels against the same oracle)."""
import json
import math

import pytest
import torch

from pyrecover_amd.optim.adamw import FlatAdamW, LossScaleGuard
from tests.test_distributed import _argv, _run


def oracle(events, scale, interval, dynamic=True):
    """The issue's rule, one line per state: events are True (finite gradient) / False."""
    tracker = applied = skipped = consecutive = 0
    for ok in events:
        if not ok:
            skipped, consecutive = skipped + 1, consecutive + 1
            if dynamic:
                scale, tracker = scale * 0.5, 0
        else:
            applied, consecutive = applied + 1, 0
            if dynamic:
                tracker += 1
                if tracker == interval:
                    scale, tracker = scale * 2.0, 0
    return {"scale": scale, "tracker": tracker, "applied": applied, "skipped_total": skipped,
            "consecutive_skips": consecutive}


SEQUENCE = [True, True, True, False, True, False, False]  # ok ok ok (grow) bad (halve) ok bad bad


@pytest.mark.parametrize("dynamic", [True, False])
def test_state_machine_matches_oracle(dynamic):
    g = LossScaleGuard(torch.device("cpu"), dynamic=dynamic, init_scale=1024.0, growth_interval=3)
    grad = torch.full((7,), 0.5)
    for i, ok in enumerate(SEQUENCE, 1):
        x = grad * float(g.scale_dev[0])
        if not ok:
            x[i % 7] = float("inf") if i % 2 else float("nan")
        s = float(g.scale_dev[0])
        g.run(x, pre_scale=0.25)
        r = g.read()
        want = oracle(SEQUENCE[:i], 1024.0, 3, dynamic)
        assert {k: r[k] for k in want} == want, (i, r, want)
        assert r["found"] == (0 if ok else 1)
        if ok:
            assert float(g.multiplier[0]) == 1.0 / s  # no clipping: exactly 1 / scale
            assert r["grad_norm"] == pytest.approx(0.25 * math.sqrt(7 * 0.25), rel=1e-6)  # the unscaled norm
        else:
            assert float(g.multiplier[0]) == 0.0 and not math.isfinite(r["grad_norm"])
    if dynamic:
        assert g.read()["scale"] == 1024.0 * 2 * 0.5 * 0.5 * 0.5


def test_guard_clips_on_the_unscaled_norm():
    g = LossScaleGuard(torch.device("cpu"), dynamic=False, init_scale=256.0, max_norm=0.5)
    g.run(torch.full((4,), 256.0), pre_scale=1.0)  # unscaled gradient of ones: norm 2
    assert g.read()["grad_norm"] == 2.0
    assert float(g.multiplier[0]) == pytest.approx(0.5 / (2.0 + 1e-6) / 256.0, rel=1e-6)


def _tiny_opt(dtype, master):
    from pyrecover_amd.config import get_preset
    from pyrecover_amd.models.llama import Transformer

    torch.manual_seed(0)
    m = Transformer(get_preset("llama-micro", seq_len=32, n_layers=1)).to(dtype)
    flat = m.flatten_()
    opt = FlatAdamW(flat, lr=1e-2, master_weights=master)
    return flat, opt


@pytest.mark.parametrize("dtype,master", [(torch.float32, False), (torch.float64, False), (torch.bfloat16, True)])
def test_step_reference_skip_leaves_everything_unchanged(dtype, master):
    flat, opt = _tiny_opt(dtype, master)
    guard = LossScaleGuard(flat.data.device, dynamic=True, init_scale=8.0, growth_interval=100)
    opt.enable_guard(guard)
    gen = torch.Generator().manual_seed(1)

    def step(poison):
        flat.grad.copy_(torch.randn(flat.numel, generator=gen).to(dtype) * 8.0)
        if poison is not None:
            flat.grad[flat.numel // 2] = poison
        guard.run(flat.grad, pre_scale=1.0)
        opt.step()

    step(None)  # non-zero moments
    assert opt.applied_steps() == 1
    bufs = [flat.data, opt.exp_avg, opt.exp_avg_sq] + ([opt.master] if master else [])
    assert (opt.master is not None) == master
    for poison in (float("inf"), float("nan")):
        keep = [b.clone() for b in bufs]
        step(poison)
        for b, k in zip(bufs, keep):
            assert torch.equal(b, k)
        assert opt.applied_steps() == 1
    assert guard.read()["skipped_total"] == 2 and guard.read()["scale"] == 2.0
    keep = flat.data.clone()
    step(None)
    assert opt.applied_steps() == 2 and not torch.equal(flat.data, keep)
    assert float(opt.state_dict()["state"][0]["step"]) == 2.0


def test_guarded_update_equals_plain_update_on_unscaled_gradient():
    """Scale 2^k: (g * s) * (1 / s) is exact, and the bias corrections follow the applied count, so a
    guarded run with a skipped step in the middle equals a plain run without that step."""
    runs = []
    for guarded in (False, True):
        flat, opt = _tiny_opt(torch.float32, False)
        guard = LossScaleGuard(flat.data.device, dynamic=False, init_scale=4096.0)
        if guarded:
            opt.enable_guard(guard)
        gen = torch.Generator().manual_seed(3)
        for i in range(4):
            g = torch.randn(flat.numel, generator=gen)
            if guarded:
                flat.grad.copy_(g * 4096.0)
                guard.run(flat.grad)
                opt.step()
                if i == 1:  # an extra, poisoned step
                    flat.grad[5] = float("nan")
                    guard.run(flat.grad)
                    opt.step()
            else:
                flat.grad.copy_(g)
                opt.step()
        runs.append((flat.data.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------
STEPS, FAULT_STEP, INTERVAL = 12, 5, 4
LS = ["--loss-scale", "dynamic", "--loss-scale-growth-interval", str(INTERVAL)]


def _ls_argv(ckdir, extra=()):
    return _argv(ckdir, STEPS, ["--sequence-length", "64", "--checkpoint-frequency", "6"] + list(extra))


def _ckpt(path):
    return torch.load(path, weights_only=True)


def _finite(ck):
    return all(bool(torch.isfinite(v).all()) for v in ck["model"].values())


@pytest.fixture(scope="module")
def straight(tmp_path_factory):
    """The uninterrupted 12-step run with a NaN injected at step 5, shared by the tests below."""
    tmp = tmp_path_factory.mktemp("ls")
    mp = pytest.MonkeyPatch()
    mp.setenv("PYRECOVER_FAULT", f"nan_grad:{FAULT_STEP}")
    try:
        _run(1, _ls_argv(tmp / "on", LS + ["--metrics-jsonl", str(tmp / "m.jsonl"), "--logging-frequency", "1"]), tmp)
        _run(1, _ls_argv(tmp / "off"), tmp)
    finally:
        mp.undo()
    return tmp


def test_train_skips_the_poisoned_step(straight):
    ck = _ckpt(straight / "on" / "e" / f"ckpt_{STEPS}.pt")
    assert _finite(ck)
    want = oracle([s != FAULT_STEP for s in range(1, STEPS + 1)], 65536.0, INTERVAL)
    ls = ck["pyrecover_state"]["loss_scale"]
    assert ls == {k: want[k] for k in ("scale", "tracker", "applied", "skipped_total")}
    assert ls["skipped_total"] == 1
    assert {float(st["step"]) for st in ck["optimizer"]["state"].values()} == {float(STEPS - 1)}
    assert set(ck["optimizer"]["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}  # torch.optim.AdamW's keys
    recs = [json.loads(line) for line in open(straight / "m.jsonl")]
    assert [r["skipped_steps"] for r in recs] == [0] * (FAULT_STEP - 1) + [1] * (STEPS - FAULT_STEP + 1)
    assert recs[-1]["loss_scale"] == want["scale"] and math.isfinite(recs[-1]["grad_norm"])
    assert recs[FAULT_STEP - 1]["grad_norm"] is None  # the skipped step: its norm is not a number
    assert all(math.isfinite(r["loss"]) for r in recs)


def test_without_loss_scale_the_same_fault_poisons_the_parameters(straight):
    """Today's behaviour, asserted so that the test above shows the need."""
    ck = _ckpt(straight / "off" / "e" / f"ckpt_{STEPS}.pt")
    assert not _finite(ck)
    assert "loss_scale" not in ck["pyrecover_state"]


@pytest.mark.parametrize("fmt", ["vanilla", "sharded"])
def test_resume_is_bitwise(straight, tmp_path, monkeypatch, fmt):
    """Checkpointed at step 6 (after the skipped step and a change of scale) and resumed: parameters,
    moments and scaler state at step 12 equal the uninterrupted run's, in both formats."""
    monkeypatch.setenv("PYRECOVER_FAULT", f"nan_grad:{FAULT_STEP}")
    f = ["--use-torch-distributed-ckpt"] if fmt == "sharded" else []
    _run(1, _ls_argv(tmp_path / "r", LS + f + ["--stop-at-step", "6"]), tmp_path)
    _run(1, _ls_argv(tmp_path / "r", LS + f + ["--resume-from-checkpoint", "latest"]), tmp_path)
    ref = _ckpt(straight / "on" / "e" / f"ckpt_{STEPS}.pt")
    if fmt == "vanilla":
        got = _ckpt(tmp_path / "r" / "e" / f"ckpt_{STEPS}.pt")
    else:
        from pyrecover_amd.ckpt.sharded import build_ckpt, read_sharded_state

        got = build_ckpt(read_sharded_state(str(tmp_path / "r" / "e" / f"ckpt_{STEPS}")))
    for k in ref["model"]:
        assert torch.equal(ref["model"][k], got["model"][k]), k
    for i, st in ref["optimizer"]["state"].items():
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(st[k], got["optimizer"]["state"][i][k]), (i, k)
        assert float(st["step"]) == float(got["optimizer"]["state"][i]["step"]) == STEPS - 1
    gls = {k: (v.item() if isinstance(v, torch.Tensor) else v) for k, v in got["pyrecover_state"]["loss_scale"].items()}
    assert gls == ref["pyrecover_state"]["loss_scale"]


def test_checkpoint_without_scaler_state_resumes_with_cli_values(tmp_path):
    _run(1, _ls_argv(tmp_path / "c", ["--stop-at-step", "6"]), tmp_path)  # written with --loss-scale off
    _run(1, _ls_argv(tmp_path / "c", ["--loss-scale", "dynamic", "--loss-scale-init", "512",
                                      "--loss-scale-growth-interval", "100", "--resume-from-checkpoint", "latest"]),
         tmp_path)
    ck = _ckpt(tmp_path / "c" / "e" / f"ckpt_{STEPS}.pt")
    assert ck["pyrecover_state"]["loss_scale"] == {"scale": 512.0, "tracker": 6, "applied": STEPS, "skipped_total": 0}


def test_composes_with_clip_and_accumulation(tmp_path, monkeypatch):
    """--clip-grad and --grad-accumulation-steps with a fixed power-of-two scale: the unscaled norm and
    so the clip coefficient are those of the unscaled run up to rounding, and the step still skips."""
    ex = ["--clip-grad", "--grad-max-norm", "0.05", "--grad-accumulation-steps", "2"]
    _run(1, _ls_argv(tmp_path / "plain", ex), tmp_path)
    _run(1, _ls_argv(tmp_path / "scaled", ex + ["--loss-scale", "1024"]), tmp_path)
    a, b = _ckpt(tmp_path / "plain" / "e" / f"ckpt_{STEPS}.pt"), _ckpt(tmp_path / "scaled" / "e" / f"ckpt_{STEPS}.pt")
    for k in a["model"]:
        torch.testing.assert_close(a["model"][k], b["model"][k], rtol=1e-4, atol=1e-6)
    monkeypatch.setenv("PYRECOVER_FAULT", f"nan_grad:{FAULT_STEP}")
    _run(1, _ls_argv(tmp_path / "skip", ex + ["--loss-scale", "1024"]), tmp_path)
    c = _ckpt(tmp_path / "skip" / "e" / f"ckpt_{STEPS}.pt")
    assert _finite(c) and c["pyrecover_state"]["loss_scale"] == {"scale": 1024.0, "tracker": 0, "applied": STEPS - 1,
                                                                 "skipped_total": 1}


def test_two_ranks_skip_together(tmp_path, monkeypatch):
    """gloo W=2, the NaN on rank 1 only: it reaches rank 0 through the gradient reduction, both ranks
    skip step 5 (the replica check at every step passes), and the all-reduce and the sharded
    optimizer end bitwise equal."""
    monkeypatch.setenv("PYRECOVER_FAULT", f"nan_grad:{FAULT_STEP}:1")
    ex = LS + ["--distributed", "--replica-check-every", "1", "--checkpoint-frequency", str(STEPS)]
    _run(2, _ls_argv(tmp_path / "ar", ex), tmp_path)
    _run(2, _ls_argv(tmp_path / "zero", ex + ["--shard-optimizer", "on"]), tmp_path)
    a, z = _ckpt(tmp_path / "ar" / "e" / f"ckpt_{STEPS}.pt"), _ckpt(tmp_path / "zero" / "e" / f"ckpt_{STEPS}.pt")
    want = oracle([s != FAULT_STEP for s in range(1, STEPS + 1)], 65536.0, INTERVAL)
    for ck in (a, z):
        assert _finite(ck)
        assert ck["pyrecover_state"]["loss_scale"] == {k: want[k] for k in ("scale", "tracker", "applied", "skipped_total")}
    assert z["pyrecover_state"]["reduction"]["shard_optimizer"] is True
    for k in a["model"]:
        assert torch.equal(a["model"][k], z["model"][k]), k
    for i, st in a["optimizer"]["state"].items():
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(st[k], z["optimizer"]["state"][i][k]), (i, k)


def test_consecutive_skips_end_the_run(tmp_path, monkeypatch):
    import pyrecover_amd.trainer as T

    monkeypatch.setattr(T, "MAX_CONSECUTIVE_SKIPS", 1)
    monkeypatch.setenv("PYRECOVER_FAULT", "nan_grad:2")
    with pytest.raises(RuntimeError, match="skipped"):
        _run(1, _ls_argv(tmp_path / "x", LS + ["--logging-frequency", "1"]), tmp_path)


def test_cli_values():
    from pyrecover_amd.cli import get_args

    assert get_args([]).loss_scale == "off"
    assert get_args(["--loss-scale", "dynamic"]).loss_scale == "dynamic"
    assert get_args(["--loss-scale", "128"]).loss_scale == 128.0
    for bad in ("0", "-1", "nan", "inf", "on"):
        with pytest.raises(SystemExit):
            get_args(["--loss-scale", bad])
