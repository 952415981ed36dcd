"""--stochastic-rounding on the CPU: the Philox bit source, the rounding rule (pyrecover_amd/optim/sr.py,
the oracle of the HIP kernels in tests/test_stochastic_rounding_gpu.py), and the feature through
FlatAdamW and train.py: drift, resume, seeds, the guard, two gloo ranks."""
import math

import pytest
import torch

from pyrecover_amd.optim import sr
from pyrecover_amd.optim.adamw import FlatAdamW, LossScaleGuard
from pyrecover_amd.parallel.flat import FlatParams
from tests.test_distributed import _argv, _run

KAT = [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


@pytest.mark.parametrize("counter,key,want", KAT)
def test_philox_known_answers(counter, key, want):
    out = sr.philox4x32_10(counter, key)
    assert " ".join(f"{int(w):08x}" for w in out) == want


def test_philox_is_elementwise_over_tensors():
    c = [torch.tensor([k[0][i] for k in KAT]) for i in range(4)]
    for row, (counter, key, want) in enumerate(KAT):
        out = sr.philox4x32_10(c, key)
        assert " ".join(f"{int(w[row]):08x}" for w in out) == want


def test_random16_layout():
    """Position idx: chunk g = idx >> 3 -> counter (g lo, g hi, t, stream), key (seed lo, seed hi);
    lane = idx & 7 -> word lane >> 1, low half for even lanes, high half for odd ones."""
    seed, t = 0x299F31D0A4093822, 0x13198A2E
    g = 0x05A308D3243F6A88 >> 3  # a chunk index with a non-zero high word
    idx = torch.arange(8, dtype=torch.int64) + (g << 3)
    for stream in (0, 1, 2):
        words = [int(w) for w in sr.philox4x32_10((g & 0xFFFFFFFF, g >> 32, t, stream),
                                                  (seed & 0xFFFFFFFF, seed >> 32))]
        want = [(words[lane >> 1] >> (16 * (lane & 1))) & 0xFFFF for lane in range(8)]
        assert sr.random16(idx, t, stream, seed).tolist() == want
    # the first known answer is position 0..7, step 0, stream 0, seed 0
    w = [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert sr.random16(torch.arange(8), 0, 0, 0).tolist() == [(w[i >> 1] >> (16 * (i & 1))) & 0xFFFF for i in range(8)]
    # different positions, steps, streams and seeds give different bits
    base = sr.random16(torch.arange(4096), 1, 0, 1)
    for other in (sr.random16(torch.arange(4096) + 4096, 1, 0, 1), sr.random16(torch.arange(4096), 2, 0, 1),
                  sr.random16(torch.arange(4096), 1, 1, 1), sr.random16(torch.arange(4096), 1, 0, 2),
                  sr.random16(torch.arange(4096), 1, 0, 1 + (1 << 32))):
        assert (base != other).float().mean() > 0.99


# ------------------------------------------------------------------------------------------------
def _bits16(x):
    return x.view(torch.int16).to(torch.int64) & 0xFFFF


def _from_bits16(b, dtype):
    b = torch.as_tensor(b, dtype=torch.int64)
    return torch.where(b >= 0x8000, b - 0x10000, b).to(torch.int16).view(dtype)


def _lo_hi(x, dtype):
    """lo: x truncated toward zero to dtype; hi: the next dtype value away from zero (fp64 search over
    the neighbours of the plain cast, independent of sr.py's arithmetic)."""
    c = _bits16(x.to(dtype))
    mag = c & 0x7FFF
    sign = c & 0x8000
    cands = [(mag + d).clamp(0, 0x7C00 if dtype == torch.float16 else 0x7F80) for d in (-1, 0, 1)]
    vals = [_from_bits16(m | sign, dtype).double().abs() for m in cands]
    ax = x.double().abs()
    lo = torch.zeros_like(ax)
    lo_bits = torch.zeros_like(mag)
    for m, v in zip(cands, vals):  # ascending magnitudes: the largest one not above |x|
        ok = v <= ax
        lo = torch.where(ok, v, lo)
        lo_bits = torch.where(ok, m, lo_bits)
    return lo_bits | sign, (lo_bits + 1) | sign


def _sample(dtype, n=20000):
    g = torch.Generator().manual_seed(5)
    top = 4.0 if dtype == torch.float16 else 30.0
    low = -8.5 if dtype == torch.float16 else -30.0  # fp16: down through its subnormals (below 2^-14 ~ 6e-5)
    x = torch.randn(n, generator=g) * 10.0 ** (torch.rand(n, generator=g) * (top - low) + low)
    return x.float()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_stochastic_round_properties(dtype):
    idx = torch.arange(20000)
    x = _sample(dtype)
    y = sr.stochastic_round(x, dtype, idx, 3, 0, 11)
    assert y.dtype == dtype and y.shape == x.shape
    # always lo or hi, both occur
    lo, hi = _lo_hi(x, dtype)
    yb = _bits16(y)
    assert bool(((yb == lo) | (yb == hi)).all())
    inexact = _from_bits16(lo, dtype).float() != x
    assert (yb == lo)[inexact].any() and (yb == hi)[inexact].any()
    # representable inputs are unchanged whatever the bits, -0 included
    rep = torch.cat([y.float(), torch.tensor([0.0, -0.0, 1.0, -1.0])])
    for t in (1, 2):
        out = sr.stochastic_round(rep, dtype, torch.arange(rep.numel()), t, 1, 99)
        assert torch.equal(_bits16(out), _bits16(rep.to(dtype)))
    # negative values mirror positive ones (same positions, so the same bits)
    neg = sr.stochastic_round(-x, dtype, idx, 3, 0, 11)
    assert torch.equal(_bits16(neg), yb ^ 0x8000)
    # NaN, inf and values beyond the largest finite one: the plain cast
    big = torch.finfo(dtype).max
    edge = torch.tensor([float("nan"), float("inf"), -float("inf"), big * (1 + 2.0 ** -12), -big * (1 + 2.0 ** -12),
                         big * 1.5, 3.4e38, -3.4e38], dtype=torch.float32)
    for t in range(1, 9):
        out = sr.stochastic_round(edge, dtype, torch.arange(8), t, 0, 7)
        want = edge.to(dtype)
        assert torch.equal(torch.isnan(out), torch.isnan(want))
        assert torch.equal(_bits16(out)[1:], _bits16(want)[1:])
    # the largest finite value itself, and just below it, stay finite
    near = torch.tensor([big, -big, big * (1 - 2.0 ** -12)], dtype=torch.float32)
    for t in range(1, 9):
        assert bool(torch.isfinite(sr.stochastic_round(near, dtype, torch.arange(3), t, 0, 7).float()).all())


def test_fp16_subnormal_results():
    """Below 2^-14 fp16's step is 2^-24: x = (k + f) * 2^-24 rounds to k or k + 1 steps with
    probability f, up into the smallest normal at k = 1023, and tiny values mostly to (signed) zero."""
    n = 65536
    idx = torch.arange(n)
    for k, f in ((0, 0.25), (3, 0.5), (700, 0.75), (1023, 0.5)):
        x = torch.full((n,), (k + f) * 2.0 ** -24, dtype=torch.float32)
        for s in (1.0, -1.0):
            y = sr.stochastic_round(x * s, torch.float16, idx, 5, 2, 3)
            steps = y.double() * s / 2.0 ** -24
            assert bool(((steps == k) | (steps == k + 1)).all())
            up = (steps == k + 1).double().mean().item()
            assert abs(up - f) < 4 * math.sqrt(f * (1 - f) / n)
            assert bool((torch.signbit(y) == (s < 0)).all())
    tiny = torch.full((n,), -1e-30, dtype=torch.float32)  # tfrac = 0: always -0
    y = sr.stochastic_round(tiny, torch.float16, idx, 1, 0, 3)
    assert bool((y == 0).all()) and bool(torch.signbit(y).all())


@pytest.mark.parametrize("stream", [0, 1, 2])
def test_rounding_frequencies_bf16(stream):
    """Seed 42, t 7, positions 0..65535: the share rounded away from zero is frac / 65536 within 4
    binomial standard deviations (deterministic)."""
    n = 65536
    idx = torch.arange(n)
    g = torch.Generator().manual_seed(2)
    base = (torch.randn(n, generator=g) * 3).to(torch.bfloat16).float()
    base = torch.where(base == 0, torch.ones_like(base), base)
    for frac in (0x4000, 0x0100, 0xFF00, 0x8000):
        x = ((base.view(torch.int32).to(torch.int64) & 0xFFFFFFFF) | frac)
        x = torch.where(x >= 1 << 31, x - (1 << 32), x).to(torch.int32).view(torch.float32)
        y = sr.stochastic_round(x, torch.bfloat16, idx, 7, stream, 42)
        away = (y.float().abs() > x.abs()).double().mean().item()
        p = frac / 65536
        sd = math.sqrt(p * (1 - p) / n)
        print(f"stream {stream} frac {frac:#06x}: share {away:.5f} want {p:.5f} ({(away - p) / sd:+.2f} sd)")
        assert abs(away - p) <= 4 * sd


def test_rounding_frequencies_fp16():
    n = 65536
    idx = torch.arange(n)
    for frac13 in (0x0800, 0x1000, 0x0020):
        x = torch.full((n,), 1.5) .view(torch.int32) | frac13  # 1.5 + frac13 * 2^-23; fp16 keeps 10 bits
        y = sr.stochastic_round(x.view(torch.float32), torch.float16, idx, 7, 0, 42)
        away = (y.float() > x.view(torch.float32)).double().mean().item()
        p = frac13 / 8192
        assert abs(away - p) <= 4 * math.sqrt(p * (1 - p) / n)


# ------------------------------------------------------------------------------------------------
N, STEPS_DRIFT = 4096, 512


def drift_run(device, mode, master=False):
    """4096 parameters at 1.0, constant gradient 1, lr 2^-12, wd 0, betas (0.9, 0.999), 512 steps."""
    p = torch.nn.Parameter(torch.ones(N, dtype=torch.bfloat16, device=device))
    flat = FlatParams([[("p", p)]])
    opt = FlatAdamW(flat, lr=2.0 ** -12, weight_decay=0.0, betas=(0.9, 0.999), master_weights=master)
    if mode != "off":
        opt.enable_stochastic_rounding(mode, 42)
    for _ in range(STEPS_DRIFT):
        flat.grad.fill_(1.0)
        opt.step()
    return (opt.master if master else flat.data)[:N].double().cpu()


def test_drift_rne_stalls_and_sr_tracks_fp32():
    rne = drift_run("cpu", "off")
    assert bool((rne == 1.0).all())  # every update is below half a bf16 ulp of 1.0: lost, every step
    ref = drift_run("cpu", "off", master=True).mean().item()
    got = drift_run("cpu", "all").mean().item()
    print(f"fp32 master mean {ref:.6f}  SR all mean {got:.6f}  diff {got - ref:+.2e}")
    assert abs(ref - 0.875) < 1e-3
    # 15 binomial sd of the mean (sd 3.3e-4), against a drift of 0.125
    assert abs(got - ref) < 0.005


def test_rejected_combinations():
    p = torch.nn.Parameter(torch.ones(64, dtype=torch.bfloat16))
    opt = FlatAdamW(FlatParams([[("p", p)]]), master_weights=True)
    with pytest.raises(ValueError, match="master"):
        opt.enable_stochastic_rounding("all", 1)
    for dt in (torch.float32, torch.float64):
        p = torch.nn.Parameter(torch.ones(64, dtype=dt))
        opt = FlatAdamW(FlatParams([[("p", p)]]))
        with pytest.raises(ValueError, match="bf16 or fp16"):
            opt.enable_stochastic_rounding("params", 1)
    p = torch.nn.Parameter(torch.ones(64, dtype=torch.float16))
    opt = FlatAdamW(FlatParams([[("p", p)]]))
    with pytest.raises(ValueError, match="mode"):
        opt.enable_stochastic_rounding("moments", 1)
    opt.enable_stochastic_rounding("params", 5)
    assert (opt.sr_mask, opt.sr_seed) == (1, 5)
    opt.enable_stochastic_rounding("all", 6)
    assert (opt.sr_mask, opt.sr_seed) == (7, 6)


def test_update_uses_the_documented_positions_and_step():
    """FlatAdamW on the CPU rounds element i of the flat buffer with the bits of (seed, step, i, tensor):
    recomputed here from the RNE-free fp32 update of one step."""
    n = 200
    outs = []
    for mode in ("off", "params", "all"):
        torch.manual_seed(0)
        p = torch.nn.Parameter(torch.randn(n).to(torch.bfloat16))
        flat = FlatParams([[("p", p)]])
        opt = FlatAdamW(flat, lr=1e-2)
        if mode != "off":
            opt.enable_stochastic_rounding(mode, 9)
        g = torch.Generator().manual_seed(1)
        for _ in range(2):
            flat.grad.copy_(torch.randn(flat.numel, generator=g).to(torch.bfloat16))
            before = [t.clone() for t in (flat.data, opt.exp_avg, opt.exp_avg_sq)]
            opt.step()
        outs.append((before, [t.clone() for t in (flat.data, opt.exp_avg, opt.exp_avg_sq)], flat.grad.clone()))
    # the fp32 values of step 2, from the state before it
    (p0, m0, v0), got, g = outs[2]
    lr, b1, b2, eps, wd = 1e-2, 0.9, 0.999, 1e-8, 1e-2
    gr = g.float()
    p = p0.float().mul(1 - lr * wd)
    m = m0.float().lerp(gr, 1 - b1)
    v = v0.float().mul(b2).addcmul(gr, gr, value=1 - b2)
    p = p.addcdiv(m, v.sqrt().div(math.sqrt(1 - b2 ** 2)).add(eps), value=-(lr / (1 - b1 ** 2)))
    idx = torch.arange(p.numel())
    for val, stream, have in zip((p, m, v), (0, 1, 2), got):
        assert torch.equal(sr.stochastic_round(val, torch.bfloat16, idx, 2, stream, 9), have)
    # params mode: p from stream 0, the moments round to nearest
    (p0, m0, v0), got, g = outs[1]
    gr = g.float()
    assert torch.equal(m0.float().lerp(gr, 1 - b1).to(torch.bfloat16), got[1])
    assert not torch.equal(outs[0][1][0], outs[1][1][0])  # and SR moved something RNE did not


# ------------------------------------------------------------------------------------------------
def _guarded(skip_at):
    torch.manual_seed(0)
    p = torch.nn.Parameter(torch.randn(1000).to(torch.bfloat16))
    flat = FlatParams([[("p", p)]])
    opt = FlatAdamW(flat, lr=1e-2)
    opt.enable_stochastic_rounding("all", 3)
    guard = LossScaleGuard(flat.data.device, dynamic=False, init_scale=64.0)
    opt.enable_guard(guard)
    gen = torch.Generator().manual_seed(1)
    for i in range(4):
        g = torch.randn(flat.numel, generator=gen).to(torch.bfloat16)
        flat.grad.copy_(g * 64.0)
        guard.run(flat.grad)
        opt.step()
        if i == skip_at:
            keep = [t.clone() for t in (flat.data, opt.exp_avg, opt.exp_avg_sq)]
            flat.grad[17] = float("nan")
            guard.run(flat.grad)
            opt.step()
            for t, k in zip((flat.data, opt.exp_avg, opt.exp_avg_sq), keep):
                assert torch.equal(t, k)  # a skipped step: nothing moves
    return flat.data.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.applied_steps()


def test_guard_skip_consumes_no_random_numbers():
    a, b = _guarded(None), _guarded(1)
    assert a[3] == b[3] == 4
    for x, y in zip(a[:3], b[:3]):
        assert torch.equal(x, y)  # the step after the skip drew the bits of t = 3, as without the skip


# ------------------------------------------------------------------------------------------------
STEPS = 6
SR = ["--model-dtype", "bf16", "--sequence-length", "64", "--checkpoint-frequency", "3", "--stochastic-rounding", "all"]


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


@pytest.fixture(scope="module")
def straight(tmp_path_factory):
    """The uninterrupted 6-step run with --stochastic-rounding all --sr-seed 1."""
    tmp = tmp_path_factory.mktemp("sr")
    _run(1, _argv(tmp / "s1", STEPS, SR + ["--sr-seed", "1"]), tmp)
    return tmp


def test_checkpoint_records_mode_and_seed(straight, tmp_path):
    ck = _ckpt(straight / "s1" / "e" / f"ckpt_{STEPS}.pt")
    assert ck["pyrecover_state"]["stochastic_rounding"] == {"mode": "all", "seed": 1}
    assert set(ck["optimizer"]["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}  # torch.optim.AdamW's keys
    assert ck["optimizer"]["state"][0]["exp_avg"].dtype == torch.bfloat16
    # default seed: --seed; off: no key
    _run(1, _argv(tmp_path / "d", 1, SR + ["--checkpoint-frequency", "1", "--seed", "77"]), tmp_path)
    assert _ckpt(tmp_path / "d" / "e" / "ckpt_1.pt")["pyrecover_state"]["stochastic_rounding"] == {"mode": "all", "seed": 77}
    _run(1, _argv(tmp_path / "o", 1, ["--model-dtype", "bf16", "--sequence-length", "64", "--checkpoint-frequency", "1"]),
         tmp_path)
    assert "stochastic_rounding" not in _ckpt(tmp_path / "o" / "e" / "ckpt_1.pt")["pyrecover_state"]


def test_seeds(straight, tmp_path):
    _run(1, _argv(tmp_path / "again", STEPS, SR + ["--sr-seed", "1"]), tmp_path)
    _run(1, _argv(tmp_path / "other", STEPS, SR + ["--sr-seed", "2"]), tmp_path)
    ref = _ckpt(straight / "s1" / "e" / f"ckpt_{STEPS}.pt")
    _same_state(ref, _ckpt(tmp_path / "again" / "e" / f"ckpt_{STEPS}.pt"))
    _same_state(ref, _ckpt(tmp_path / "other" / "e" / f"ckpt_{STEPS}.pt"), equal=False)


@pytest.mark.parametrize("fmt", ["vanilla", "sharded"])
def test_resume_is_bitwise(straight, tmp_path, fmt):
    """3 steps + resume + 3 steps equal 6 steps; the resumed run is started with another --sr-seed and
    takes the checkpoint's."""
    f = ["--use-torch-distributed-ckpt"] if fmt == "sharded" else []
    _run(1, _argv(tmp_path / "r", STEPS, SR + f + ["--sr-seed", "1", "--stop-at-step", "3"]), tmp_path)
    _run(1, _argv(tmp_path / "r", STEPS, SR + f + ["--sr-seed", "5", "--resume-from-checkpoint", "latest"]), tmp_path)
    ref = _ckpt(straight / "s1" / "e" / f"ckpt_{STEPS}.pt")
    if fmt == "vanilla":
        got = _ckpt(tmp_path / "r" / "e" / f"ckpt_{STEPS}.pt")
    else:
        from pyrecover_amd.ckpt.sharded import build_ckpt, read_sharded_state

        got = build_ckpt(read_sharded_state(str(tmp_path / "r" / "e" / f"ckpt_{STEPS}")))
    _same_state(ref, got)
    srs = got["pyrecover_state"]["stochastic_rounding"]
    assert {k: (v.item() if isinstance(v, torch.Tensor) else v) for k, v in srs.items()} == {"mode": "all", "seed": 1}


def test_resume_with_another_mode_keeps_the_flag(straight, tmp_path):
    _run(1, _argv(tmp_path / "m", STEPS, SR + ["--sr-seed", "1", "--stop-at-step", "3"]), tmp_path)
    _run(1, _argv(tmp_path / "m", STEPS, SR + ["--stochastic-rounding", "params", "--resume-from-checkpoint", "latest"]),
         tmp_path)
    ck = _ckpt(tmp_path / "m" / "e" / f"ckpt_{STEPS}.pt")
    assert ck["pyrecover_state"]["stochastic_rounding"] == {"mode": "params", "seed": 1}


def test_two_ranks_zero1_equals_allreduce(tmp_path):
    """gloo W=2, 10 steps: the sharded optimizer and the all-reduce end bitwise equal (parameters and
    moments), and the replica check at every step passes: the bits depend on neither rank nor bucket."""
    ex = SR + ["--sr-seed", "4", "--distributed", "--replica-check-every", "1", "--checkpoint-frequency", "10"]
    _run(2, _argv(tmp_path / "ar", 10, ex + ["--shard-optimizer", "off"]), tmp_path)
    _run(2, _argv(tmp_path / "zero", 10, ex + ["--shard-optimizer", "on"]), tmp_path)
    a, z = _ckpt(tmp_path / "ar" / "e" / "ckpt_10.pt"), _ckpt(tmp_path / "zero" / "e" / "ckpt_10.pt")
    assert z["pyrecover_state"]["reduction"]["shard_optimizer"] is True
    assert a["pyrecover_state"]["reduction"]["shard_optimizer"] is False
    _same_state(a, z)


def test_cli_rejects_master_weights_and_fp32(tmp_path):
    with pytest.raises(ValueError, match="master"):
        _run(1, _argv(tmp_path / "a", 1, SR + ["--master-weights", "fp32"]), tmp_path)
    with pytest.raises(ValueError, match="bf16 or fp16"):
        _run(1, _argv(tmp_path / "b", 1, SR + ["--model-dtype", "fp32"]), tmp_path)


def test_cli_values():
    from pyrecover_amd.cli import get_args

    a = get_args([])
    assert a.stochastic_rounding == "off" and a.sr_seed is None
    a = get_args(["--stochastic-rounding", "params", "--sr-seed", "9"])
    assert a.stochastic_rounding == "params" and a.sr_seed == 9
    with pytest.raises(SystemExit):
        get_args(["--stochastic-rounding", "moments"])
