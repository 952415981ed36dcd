"""--loss-scale on the GPU: the guard kernel, the skip flag of the four AdamW kernels, torch's fused
AdamW with grad_scale / found_inf as the bitwise oracle, and the trained model eager and replayed.
The state-machine oracle is tests/test_loss_scale.py's."""
import json
import math

import pytest
import torch

from pyrecover_amd import _ext
from pyrecover_amd.optim.adamw import FlatAdamW, LossScaleGuard
from tests import kernel_oracles as K
from tests.test_loss_scale import oracle

pytestmark = pytest.mark.gpu

LR, B1, B2, AEPS, WD = 1e-3, 0.9, 0.999, 1e-8, 0.01
# sumsq_kernel: 1024 blocks x 256 threads x 8 elements = 2^21 per loop trip. 2^21 + 3 ends in a scalar
# tail of 3 right after the first trip; 2^21 + 11 is the smallest size with a (one-chunk) second trip
# AND a tail, so the "second trip" position (index 2^21) is a tail element at the first and a vector
# element of the second trip at the second.
GUARD_SIZES = [1, 7, 4099, (1 << 21) + 3, (1 << 21) + 11]


def _hyper(cuda):
    return torch.zeros(3, dtype=torch.float64, device=cuda)


@pytest.mark.parametrize("n", GUARD_SIZES)
@pytest.mark.parametrize("dtype", K.DTYPES, ids=K.dname)
def test_guard_kernel(cuda, n, dtype):
    """A single inf and a single NaN at element 0, at an element of the second loop trip (n // 2 where there
    is none) and at the last element: found, multiplier 0, state as the oracle's. Clean data in between:
    the unscaled norm within grad_norm's 1e-3 of the fp64 oracle, the multiplier clip / s, the bias
    corrections those of the applied count."""
    pre, interval, s0 = K.GRAD_NORM_PRE_SCALE, 2, 8.0
    x = K.grad_norm_input(n, dtype, cuda)
    o = x.double().norm().item() * pre
    positions = sorted({0, (1 << 21) if n > (1 << 21) else n // 2, n - 1})
    events = []
    g = LossScaleGuard(cuda, dynamic=True, init_scale=s0, growth_interval=interval)
    g.hyper = _hyper(cuda)
    g.betas = (B1, B2)
    plan = [(None, None, 0.0), (None, None, 0.25)]  # clean, clean + clipping (the scale doubles)
    for pos in positions:
        plan += [(pos, float("inf"), 0.0), (None, None, 0.0), (pos, float("nan"), 0.25)]
    plan += [(None, None, 0.0)]
    for pos, bad, clip_frac in plan:
        y = x
        if pos is not None:
            y = x.clone()
            y[pos] = bad
        s = g.read()["scale"]
        g.max_norm = clip_frac * o / s
        g.run(y, pre_scale=pre)
        events.append(pos is None)
        r = g.read()
        want = oracle(events, s0, interval)
        print(f"ERR guard n={n} pos={pos} bad={bad} norm={r['grad_norm']:.9e} oracle={o / s:.9e} "
              f"mult={float(g.multiplier[0]):.9e} state={r}")
        assert {k: r[k] for k in want} == want, (pos, bad, r, want)
        assert r["found"] == (0 if pos is None else 1)
        if pos is not None:
            assert float(g.multiplier[0]) == 0.0 and not math.isfinite(r["grad_norm"])
            continue
        assert abs(r["grad_norm"] - o / s) <= 1e-3 * o / s
        if clip_frac:
            wantm = g.max_norm / (o / s + 1e-6) / s
            assert abs(float(g.multiplier[0]) - wantm) <= 1e-3 * wantm
        else:
            assert float(g.multiplier[0]) == 1.0 / s  # exact: s is a power of two
        h = g.hyper.tolist()
        assert h[1] == pytest.approx(1 - B1 ** r["applied"], rel=1e-14)
        assert h[2] == pytest.approx(math.sqrt(1 - B2 ** r["applied"]), rel=1e-14)
    assert g.read()["skipped_total"] == 2 * len(positions)


def test_guard_kernel_from_a_squared_norm(cuda):
    """The sharded optimizer's entry: the all-reduced squared norm (fp64) instead of the gradient."""
    g = LossScaleGuard(cuda, dynamic=True, init_scale=4.0, growth_interval=100)
    g.hyper = _hyper(cuda)
    for sq, ok in ((36.0, True), (float("inf"), False), (float("nan"), False), (1e300, True)):
        s = g.read()["scale"]
        g.run(sq=torch.tensor([sq], dtype=torch.float64, device=cuda), pre_scale=0.5)
        r = g.read()
        assert r["found"] == (0 if ok else 1)
        assert float(g.multiplier[0]) == (1.0 / s if ok else 0.0)
        if sq == 36.0:
            assert r["grad_norm"] == 6.0 * 0.5 / 4.0
    assert g.read() | {"grad_norm": 0} == {"scale": 1.0, "tracker": 1, "found": 0, "applied": 2, "skipped_total": 2,
                                           "consecutive_skips": 0, "grad_norm": 0}


# ------------------------------------------------------------------------------------------------
OFF, PAD = 192, 333  # guard elements before and after every slice (OFF: 16-B aligned for the tiled kernel)
SKIP_CASES = [("flat", d, (4099,)) for d in K.DTYPES] + [(k, d, sh) for d in (torch.bfloat16, torch.float16)
                                                         for k, sh in (("master", (4099,)), ("t", (128, 256)),
                                                                       ("t", (64, 192)))]


def _skip_state(kind, dtype, shape, cuda):
    n = math.prod(shape)
    gen = torch.Generator(device=cuda).manual_seed(n)
    total = OFF + n + PAD
    sdt = torch.float32 if kind == "master" else dtype
    bufs = {"p": torch.randn(total, device=cuda, generator=gen).to(dtype),
            "g": (torch.randn(total, device=cuda, generator=gen) * 0.1).to(dtype),
            "m": (torch.randn(total, device=cuda, generator=gen) * 1e-3).to(sdt),
            "v": (torch.rand(total, device=cuda, generator=gen) * 1e-4).to(sdt)}
    if kind == "master":
        bufs["pm"] = bufs["p"].float()
    if kind == "t":
        bufs["pt"] = torch.zeros(total, device=cuda, dtype=dtype)
        bufs["pt"][OFF:OFF + n].view(shape[1], shape[0]).copy_(bufs["p"][OFF:OFF + n].view(shape).t())
    return bufs


def _skip_run(C, kind, shape, bufs, skip_dev):
    n = math.prod(shape)
    sl = {k: t[OFF:OFF + n] for k, t in bufs.items()}
    tail = (LR, B1, B2, AEPS, WD, 1 - B1 ** 2, math.sqrt(1 - B2 ** 2), 0.5, None, None, False, skip_dev)
    if kind == "master":
        C.adamw_master_(sl["p"], sl["pm"], sl["g"], sl["m"], sl["v"], *tail)
    elif kind == "t":
        r, c = shape
        C.adamw_t_(sl["p"].view(r, c), sl["g"].view(r, c), sl["m"].view(r, c), sl["v"].view(r, c),
                   sl["pt"].view(c, r), *tail)
    else:
        C.adamw_flat_(sl["p"], sl["g"], sl["m"], sl["v"], *tail)


@pytest.mark.parametrize("kind,dtype,shape", SKIP_CASES, ids=[f"{k}-{K.dname(d)}-{'x'.join(map(str, s))}"
                                                               for k, d, s in SKIP_CASES])
def test_skip_flag(cuda, kind, dtype, shape):
    """*skip_dev = 1: parameters, moments, master and transposed shadow bit-unchanged, slice and guard
    elements alike. *skip_dev = 0: bitwise the launch without a skip_dev."""
    C = _ext.native()
    n = math.prod(shape)
    base = _skip_state(kind, dtype, shape, cuda)
    flag = torch.ones(1, dtype=torch.int32, device=cuda)
    skipped = {k: t.clone() for k, t in base.items()}
    _skip_run(C, kind, shape, skipped, flag)
    for k in base:
        assert torch.equal(skipped[k], base[k]), k
    flag.zero_()
    zero = {k: t.clone() for k, t in base.items()}
    null = {k: t.clone() for k, t in base.items()}
    _skip_run(C, kind, shape, zero, flag)
    _skip_run(C, kind, shape, null, None)
    for k in base:
        assert torch.equal(zero[k], null[k]), k
        assert torch.equal(zero[k][:OFF], base[k][:OFF]) and torch.equal(zero[k][OFF + n:], base[k][OFF + n:]), k
        if k != "g":
            assert not torch.equal(zero[k], base[k]), k
    if kind == "t":
        r, c = shape
        assert torch.equal(zero["pt"][OFF:OFF + n].view(c, r), zero["p"][OFF:OFF + n].view(r, c).t())


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", K.DTYPES, ids=K.dname)
def test_guarded_adamw_equals_torch_fused_with_found_inf(cuda, dtype):
    """Six steps from non-zero moments, gradients pre-multiplied by 2^10, an inf in step 3: p, m and v
    bitwise equal to torch._fused_adamw_(grad_scale=, found_inf=) with its device step tensor (which
    does not advance on the skipped step, and from which torch computes the bias corrections on the
    device with fp64 pow, as the guard kernel does)."""
    C = _ext.native()
    n, scale = 4099, 1024.0
    gen = torch.Generator(device=cuda).manual_seed(7)
    p = torch.randn(n, device=cuda, generator=gen).to(dtype)
    m = (torch.randn(n, device=cuda, generator=gen) * 1e-3).to(dtype)
    v = (torch.rand(n, device=cuda, generator=gen) * 1e-4).to(dtype)
    grads = [((torch.randn(n, device=cuda, generator=gen) * 10.0 ** (-(s % 3) - 1)).to(dtype) * scale).to(dtype)
             for s in range(6)]
    grads[2][n // 3] = float("inf")
    guard = LossScaleGuard(cuda, dynamic=False, init_scale=scale)
    guard.hyper = _hyper(cuda)
    guard.betas = (B1, B2)
    guard.hyper[0] = LR
    p2, m2, v2 = p.clone(), m.clone(), v.clone()
    step = torch.zeros((), device=cuda)
    gs = torch.tensor(scale, device=cuda)
    for i, grad in enumerate(grads):
        guard.run(grad, pre_scale=1.0)
        C.adamw_flat_(p, grad, m, v, 7.0, B1, B2, AEPS, WD, 0.3, 0.3, 1.0, guard.multiplier, guard.hyper, False,
                      guard.skip_dev)
        found = (~torch.isfinite(grad.float()).all()).float()
        step += 1 - found  # torch.optim's wrapper: steps += 1, then steps -= found_inf
        torch._fused_adamw_([p2], [grad.clone()], [m2], [v2], [], [step], amsgrad=False, lr=LR, beta1=B1, beta2=B2,
                            weight_decay=WD, eps=AEPS, maximize=False, grad_scale=gs, found_inf=found)
        for name, a, b in (("p", p, p2), ("m", m, m2), ("v", v, v2)):
            bad = (a != b).nonzero()
            assert bad.numel() == 0, (i, name, bad.numel(), bad[:4].flatten().tolist())
    assert guard.read()["applied"] == 5 == int(step.item()) and guard.read()["skipped_total"] == 1
    assert bool(torch.isfinite(p.float()).all())


# ------------------------------------------------------------------------------------------------
MODEL_STEPS, MODEL_FAULT = 8, 3


def _targs(ckdir, extra=()):
    from pyrecover_amd.cli import get_args

    return get_args(["--model-preset", "llama-micro", "--synthetic-data", "--sequence-length", "128", "--batch-size", "2",
                     "--training-steps", str(MODEL_STEPS), "--checkpoint-dir", str(ckdir), "--experiment_name", "e",
                     "--checkpoint-frequency", str(MODEL_STEPS), "--num-workers", "0", "--logging-frequency", "1",
                     # (the command line's default rate: at 1e-3 the pure-fp16 run, whose second moments are
                     # fp16 too, diverges within three steps with or without a loss scale, and then overflows
                     # on its own; this test is about the one injected step)
                     "--learning-rate", "1e-5", "--lr-warmup-steps", "2", "--model-dtype", "fp16",
                     "--loss-scale", "dynamic", "--loss-scale-init", "65536", "--loss-scale-growth-interval", "4",
                     "--metrics-jsonl", str(ckdir / "m.jsonl")] + list(extra))


@pytest.mark.parametrize("extra", [[], ["--clip-grad", "--grad-max-norm", "0.5"], ["--master-weights", "fp32"]],
                         ids=["plain", "clip", "master"])
def test_model_eager_and_replayed_skip_alike(cuda, tmp_path, monkeypatch, extra):
    """llama-micro fp16, 8 steps, dynamic scale from 65536, a NaN injected at step 3 (the first replayed
    step with --compile): eager and graph replay are bitwise equal, the graph is captured once, one
    step is skipped and the scale ends where the oracle's state machine ends."""
    from pyrecover_amd.graph import StepGraph
    from pyrecover_amd.trainer import train

    monkeypatch.setenv("PYRECOVER_FAULT", f"nan_grad:{MODEL_FAULT}")
    captures = []
    orig = StepGraph._capture
    monkeypatch.setattr(StepGraph, "_capture", lambda self, *a, **k: (captures.append(1), orig(self, *a, **k))[1])
    train(_targs(tmp_path / "eager", extra))
    assert not captures
    train(_targs(tmp_path / "graph", extra + ["--compile"]))
    assert len(captures) == 1
    cks, recs = [], []
    for d in ("eager", "graph"):
        cks.append(torch.load(tmp_path / d / "e" / f"ckpt_{MODEL_STEPS}.pt", weights_only=True))
        recs.append([json.loads(line) for line in open(tmp_path / d / "m.jsonl")])
    a, b = cks
    for k in a["model"]:
        assert torch.equal(a["model"][k], b["model"][k]), k
    for i, st in a["optimizer"]["state"].items():
        for k in st:
            assert torch.equal(st[k], b["optimizer"]["state"][i][k]), (i, k)
    want = oracle([s != MODEL_FAULT for s in range(1, MODEL_STEPS + 1)], 65536.0, 4)
    for ck, rec in zip(cks, recs):
        print(f"ERR model {extra} losses={[round(r['loss'], 4) for r in rec]} scales={[r['loss_scale'] for r in rec]} "
              f"skipped={[r['skipped_steps'] for r in rec]} norms={[r['grad_norm'] for r in rec]}")
        assert ck["pyrecover_state"]["loss_scale"] == {k: want[k] for k in ("scale", "tracker", "applied", "skipped_total")}
        assert rec[-1]["skipped_steps"] == 1 and rec[-1]["loss_scale"] == want["scale"]
        assert all(math.isfinite(r["loss"]) for r in rec)
        assert all(bool(torch.isfinite(t).all()) for t in ck["model"].values())
        assert float(ck["optimizer"]["state"][0]["step"]) == MODEL_STEPS - 1
    assert [r["loss"] for r in recs[0]] == [r["loss"] for r in recs[1]]


TRACK_STEPS, TRACK_S, TRACK_B, TRACK_LR = 60, 128, 4, 3e-3  # test_model_gpu.py's micro case


@pytest.fixture(scope="module")
def torch_curve(cuda):
    """The fp32 plain-torch reference of tests/test_model_gpu.py's 60-step comparison (micro case: same
    task, seed, batches and learning rate), computed once: (initial weights, loss curve)."""
    from pyrecover_amd.config import get_preset
    from pyrecover_amd.models.llama import Transformer
    from pyrecover_amd.ops import reference as R
    from tests.test_model_gpu import ref_forward

    a = get_preset("llama-micro", seq_len=TRACK_S)
    torch.manual_seed(0)
    ref = Transformer(a).to(cuda)
    init = {k: v.clone() for k, v in ref.state_dict().items()}
    ropt = torch.optim.AdamW(ref.parameters(), lr=TRACK_LR)
    theirs = []
    for x, y in _track_batches(a, cuda):
        ropt.zero_grad()
        rl = R.cross_entropy_ref(ref_forward(ref, x), y)
        rl.backward()
        ropt.step()
        theirs.append(rl.item())
    return init, theirs


def _track_batches(a, cuda):
    gen = torch.Generator(device=cuda)
    gen.manual_seed(1)
    for _ in range(TRACK_STEPS):
        start = torch.randint(0, a.vocab_size, (TRACK_B, 1), generator=gen, device=cuda)
        seq = (start + torch.arange(TRACK_S + 1, device=cuda)) % a.vocab_size
        yield seq[:, :-1].contiguous(), seq[:, 1:].contiguous()


def _track_fp16(cuda, init, scaled, master):
    """The fp16 HIP path on the same weights and batches -> (loss curve, guard state, flat parameters)."""
    from pyrecover_amd.config import get_preset
    from pyrecover_amd.models.llama import Transformer

    a = get_preset("llama-micro", seq_len=TRACK_S)
    gpu = Transformer(a)
    gpu.load_state_dict(init)
    gpu = gpu.to(cuda, torch.float16)
    flat = gpu.flatten_()
    opt = FlatAdamW(flat, lr=TRACK_LR, master_weights=master)
    guard = None
    if scaled:
        guard = LossScaleGuard(cuda, dynamic=True, init_scale=65536.0, growth_interval=2000)
        opt.enable_guard(guard)
    ours = []
    for x, y in _track_batches(a, cuda):
        opt.zero_grad()
        loss = gpu(x, labels=y)
        if guard is not None:
            (loss * guard.scale_dev.reshape(())).backward()
            guard.run(flat.grad, pre_scale=1.0)
        else:
            loss.backward()
        opt.step()
        ours.append(loss.item())
    if guard is not None:
        assert opt.applied_steps() == guard.read()["applied"]
    return ours, (guard.read() if guard is not None else None), flat.data


def _gap(ours, theirs):
    """Largest step-by-step distance of two loss curves; a NaN loss is infinitely far."""
    return max((abs(o - t) if o == o else math.inf) for o, t in zip(ours, theirs))


def test_fp16_master_with_dynamic_scale_tracks_fp32_torch_reference(cuda, torch_curve):
    """fp16 with --master-weights fp32 under --loss-scale dynamic, held to the three bounds that
    test_training_loss_curve_tracks_fp32_torch_reference applies to the bf16 path: the scaled backward,
    the guard and the guarded master update train as the fp32 torch reference does (measured gap
    0.0009 of a bound of 0.572, no step skipped at scale 65536)."""
    init, theirs = torch_curve
    ours, st, _ = _track_fp16(cuda, init, scaled=True, master=True)
    curves = f"ours {[round(v, 3) for v in ours[::6]]} torch {[round(v, 3) for v in theirs[::6]]} guard {st}"
    gap = _gap(ours, theirs)
    print(f"ERR fp16_master_tracking gap={gap:.4f} bound={0.1 * theirs[0]:.4f} {curves}")
    assert st["applied"] + st["skipped_total"] == TRACK_STEPS
    assert abs(ours[0] - theirs[0]) < 0.02 * theirs[0], curves
    assert ours[-1] < 0.5 * ours[0] and theirs[-1] < 0.5 * theirs[0], curves
    assert gap < 0.1 * theirs[0], (gap, curves)


def _tracked(ours, theirs, bound):
    """Number of leading steps whose loss stays within `bound` of the reference; a NaN loss is outside."""
    n = 0
    for o, t in zip(ours, theirs):
        if not abs(o - t) < bound:
            break
        n += 1
    return n


def test_pure_fp16_with_dynamic_scale_is_no_worse_than_unscaled(cuda, torch_curve):
    """Pure fp16 (fp16 parameters AND fp16 moments) does not fit the existing tolerance (0.1 x the initial
    loss = 0.572) with or without a loss scale: the second moment (1 - b2) g^2 of a typical gradient
    element (|g| ~ 1e-3) is below fp16's smallest number whatever the loss scale, because the moments
    hold the unscaled gradient, so those elements step by lr * m / eps. Both runs therefore leave the
    reference within the first steps and end with losses in the thousands (measured on an MI355X: both
    follow it for 2 steps; largest distance 4359 unscaled, 4539 under --loss-scale dynamic, which skips
    13 of 60 steps and keeps loss and parameters finite). Until the dK/dV kernels stopped rounding K * scale * log2(e) to fp16, the diverged
    parameters overflowed that product and the unscaled run sat at a NaN loss from the sixth step on, which
    made `gap <= gap_plain` trivially true; between two diverged runs it is a coin toss. The scaled run is
    required to stay finite, to follow the reference for at least as many leading steps (within the
    existing tolerance) as the unscaled one, and to have no larger a gap whenever the unscaled run still
    learns anything (its gap below the loss of the untrained model; a NaN loss is infinitely far and never
    counts as learning). (fp16 that trains needs --master-weights fp32: the test above.)"""
    init, theirs = torch_curve
    plain, _, _ = _track_fp16(cuda, init, scaled=False, master=False)
    ours, st, params = _track_fp16(cuda, init, scaled=True, master=False)
    gap_plain, gap = _gap(plain, theirs), _gap(ours, theirs)
    bound = 0.1 * theirs[0]
    kept_plain, kept = _tracked(plain, theirs, bound), _tracked(ours, theirs, bound)
    print(f"ERR fp16_tracking gap_unscaled={gap_plain:.4f} gap_scaled={gap:.4f} bound={bound:.4f} "
          f"tracked_unscaled={kept_plain} tracked_scaled={kept} guard {st} "
          f"unscaled {[round(v, 3) for v in plain[:12]]} .. {[round(v, 3) for v in plain[12::6]]} "
          f"scaled {[round(v, 3) for v in ours[:12]]} .. {[round(v, 3) for v in ours[12::6]]} "
          f"torch {[round(v, 3) for v in theirs[:12]]}")
    assert abs(ours[0] - theirs[0]) < 0.02 * theirs[0]
    assert kept >= kept_plain, (kept, kept_plain)
    assert gap <= gap_plain or not gap_plain < theirs[0], (gap, gap_plain)
    assert all(math.isfinite(v) for v in ours) and bool(torch.isfinite(params.float()).all())
    assert st["applied"] + st["skipped_total"] == TRACK_STEPS
