"""AdamW over the flat parameter space, state_dict-compatible with ``torch.optim.AdamW``.

The reference builds ``torch.optim.AdamW(model.parameters(), lr, fused=--fused-optimizer)``
(reference train.py:120-122) with default betas/eps/weight_decay on all params and bf16 states
(no fp32 master copy). :class:`FlatAdamW` keeps that contract (same param_groups keys, per-param
``state[i] = {"step", "exp_avg", "exp_avg_sq"}`` in ``model.parameters()`` order), but the moments
live in two flat buffers laid out like the flat parameters, and the update is one HIP kernel
over the whole model (``pra_adamw_flat``: fp32 opmath, torch ``_fused_adamw_`` semantics).

``master_weights=True`` (``--master-weights fp32``; SURVEY §8 D18: "keep pure-bf16 as the default for
parity, optional fp32 master"): the update runs on an fp32 master copy of the parameters with fp32
moments (``pra_adamw_master``), and the 16-bit parameters the model computes with are the master
rounded once after every update. The master is saved as a third per-parameter state tensor
(``state[i]["master_param"]``) next to the fp32 moments; a checkpoint without it (pure-bf16 runs,
the reference's) resumes with the master taken from the loaded parameters.

:class:`LossScaleGuard` (``--loss-scale``) keeps a loss scale and a per-step "gradient not finite"
flag in device memory; with :meth:`FlatAdamW.enable_guard` every update kernel skips on that flag
and the step count is the number of applied updates.

:meth:`FlatAdamW.enable_stochastic_rounding` (``--stochastic-rounding``): the pure 16-bit state is
rounded stochastically instead of to nearest, with bits that are a stateless function of (seed, step,
flat position, tensor) (:mod:`pyrecover_amd.optim.sr`, ``csrc/kernels/philox_sr.h``).
"""
from __future__ import annotations

import math
import os
from typing import Optional

import torch

from .. import _ext
from ..ops import sched
from . import sr as _sr
from ..parallel.flat import FlatParams

# Matrices with a transposed weight shadow (parallel/flat.py) are updated by a tiled AdamW kernel
# that writes the shadow from the values it just computed (no transpose pass re-reading the
# weights); False (from code: tests, A/B tools) falls back to flat AdamW + a separate transpose.
FUSED_T = True
# When an overlapped bucket update is enqueued on the side stream (PYRECOVER_OPT_SCHED):
#   "attn" (default): held until the next attention backward, then enqueued behind an event recorded
#            between its dQ and dK/dV kernels (ops.sched.attention_window), so it runs beside dK/dV,
#            which leaves room on every CU and reads little from HBM;
#   "eager": as soon as the bucket is reduced (it then lands beside the register-bound dQ kernel and
#            the memory-bound SwiGLU backward and slows them).
# Same-process A/B (profiles/r3/step_ab_attnwin_*.log): 7B B16 1063.3 -> 1056.5 ms, 7B B1 99.6 ->
# 97.9 ms, Llama-3-8B S8192 B1 373.3 -> 361.5 ms, GPT-2-medium unchanged; no update at all: 1043.9
# ms at B16. (Holding the updates for the W1|W3 / QKV data-gradient GEMMs instead measured +1.45%.)
# Until a window has been seen, a bucket is held for at most one bucket: when the next bucket is
# reduced and no attention window released the held ones (a model whose attention takes the torch
# path -- fp64, head_dim not 64/128 -- or has no attention), they are enqueued then, so the update
# still overlaps the backward instead of running serialized in step().
OPT_SCHED = os.environ.get("PYRECOVER_OPT_SCHED", "attn")
# PYRECOVER_ADAMW_FAST (default 0): torch _fused_adamw_'s exact expression tree (mixed fp64/fp32,
# correctly rounded divisions; bit-equal to the reference's --fused-optimizer). 1: the
# hardware reciprocal / square root in pure fp32 (csrc/kernels/optim.hip adamw_elem<FAST>, ~17
# instead of ~60 VALU per element beside the attention backward; 7B B1 98.5 -> 97.2 ms, B16 within
# noise, profiles/r3/step_ab_fast_*.log), whose p differs from torch's by a few fp32 ulps.
FAST_MATH = os.environ.get("PYRECOVER_ADAMW_FAST", "0") == "1"


class LossScaleGuard:
    """Loss scale and non-finite step guard (``train.py --loss-scale``), state in device memory.

    ``state`` is int32[8] on the parameters' device (layout: csrc/kernels/optim.hip
    guard_finish_kernel): [0] scale (fp32 bits), [1] growth tracker, [2] found, [3] applied steps,
    [4] skipped steps, [5] consecutive skips. :meth:`run` looks at the reduced gradient once per step,
    between the backward and the update, and writes ``out`` = {unscaled norm, gradient multiplier}:

    * sum of squares not finite: the step is skipped (``skip_dev`` = 1 makes every AdamW launch a
      no-op, the multiplier is 0, the applied count stays); ``dynamic``: the scale halves;
    * else the multiplier is ``clip / scale``, ``applied`` advances (AdamW's bias corrections follow
      it, as torch's fused AdamW does with ``found_inf``); ``dynamic``: the scale doubles after
      ``interval`` consecutive applied steps. No floor and no cap, as ``torch.amp.GradScaler``.

    On the GPU this is one kernel behind the norm reduction and the host never reads the state
    except in :meth:`read` (log steps, checkpoints), so a captured step replays with it. Without a
    GPU the same rule runs in Python on the CPU tensors."""

    SCALE, TRACKER, FOUND, APPLIED, SKIPPED, CONSECUTIVE = range(6)

    def __init__(self, device, dynamic: bool = True, init_scale: float = 65536.0, growth_interval: int = 2000,
                 max_norm: float = 0.0):
        if not (init_scale > 0 and math.isfinite(init_scale)):
            raise ValueError(f"loss scale must be positive and finite, got {init_scale}")
        if int(growth_interval) < 1:
            raise ValueError("loss-scale growth interval must be at least 1")
        self.dynamic = bool(dynamic)
        self.interval = int(growth_interval)
        self.max_norm = float(max_norm)  # > 0: clip the unscaled norm to it (--clip-grad)
        self.state = torch.zeros(8, dtype=torch.int32, device=device)
        self.out = torch.zeros(2, dtype=torch.float32, device=device)
        self.scale_dev = self.state[0:1].view(torch.float32)  # fp32[1]: the backward's seed
        self.skip_dev = self.state[2:3]
        self.scale_dev.fill_(float(init_scale))
        self.hyper: Optional[torch.Tensor] = None  # the optimizer's hyper_dev (FlatAdamW.enable_guard)
        self.betas = (0.9, 0.999)
        # the HIP kernel decides; False: the same rule in Python (CPU runs, fp64 models on the GPU)
        self.native = self.state.is_cuda

    @property
    def multiplier(self) -> torch.Tensor:
        """fp32[1]: the AdamW kernels' ``gscale_dev`` (0 on a skipped step, else clip / scale)."""
        return self.out[1:2]

    def run(self, grad: Optional[torch.Tensor] = None, pre_scale: float = 1.0, sq: Optional[torch.Tensor] = None):
        """One guard step over the reduced gradient ``grad``, or over its squared norm ``sq`` (fp64[1],
        already summed over the ranks: sharded optimizer). ``pre_scale``: the gradient's static factor
        (1 / (world size x accumulation steps)), so the norm is that of the mean gradient."""
        if (grad is None) == (sq is None):
            raise ValueError("exactly one of grad and sq")
        if self.native:
            _ext.require_for(self.state).guard_step_(grad, sq, self.state, self.out, self.hyper, self.max_norm,
                                                     pre_scale, self.dynamic, self.interval, *self.betas)
            return
        if sq is None:
            sq = grad.to(torch.promote_types(grad.dtype, torch.float32)).pow(2).sum()
        sq = float(sq)
        st = self.state
        scale = float(self.scale_dev[0])
        self.out[0] = (math.sqrt(sq) if math.isfinite(sq) else sq) * pre_scale / scale
        if not math.isfinite(sq):
            self.out[1] = 0.0
            st[self.FOUND] = 1
            st[self.SKIPPED] += 1
            st[self.CONSECUTIVE] += 1
            if self.dynamic:
                self.scale_dev[0] = scale * 0.5
                st[self.TRACKER] = 0
            return
        clip = min(1.0, self.max_norm / (float(self.out[0]) + 1e-6)) if self.max_norm > 0 else 1.0
        self.out[1] = clip / scale
        st[self.FOUND] = 0
        st[self.APPLIED] += 1
        st[self.CONSECUTIVE] = 0
        if self.dynamic:
            st[self.TRACKER] += 1
            if int(st[self.TRACKER]) == self.interval:
                self.scale_dev[0] = scale * 2.0
                st[self.TRACKER] = 0

    def read(self) -> dict:
        """Host copy of the state (synchronizes with the device: log steps and checkpoints only)."""
        st = self.state.cpu()
        return {"scale": float(st[0:1].view(torch.float32)[0]), "tracker": int(st[1]), "found": int(st[2]),
                "applied": int(st[3]), "skipped_total": int(st[4]), "consecutive_skips": int(st[5]),
                "grad_norm": float(self.out[0])}

    def state_dict(self) -> dict:
        r = self.read()
        return {k: r[k] for k in ("scale", "tracker", "applied", "skipped_total")}

    def load_state_dict(self, sd: dict):
        st = torch.zeros(8, dtype=torch.int32)
        st[0:1].view(torch.float32)[0] = float(sd["scale"])
        st[self.TRACKER], st[self.APPLIED] = int(sd["tracker"]), int(sd["applied"])
        st[self.SKIPPED] = int(sd["skipped_total"])
        self.state.copy_(st)

    def set_applied(self, n: int):
        self.state[self.APPLIED:self.APPLIED + 1].fill_(int(n))


class FlatAdamW(torch.optim.AdamW):
    def __init__(self, flat: FlatParams, params=None, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 1e-2, fused: Optional[bool] = None, grad_scale: float = 1.0,
                 master_weights: bool = False):
        # default order = the model's parameters() order when the model recorded it (the
        # reference's optimizer-state indices), else the flat buffer order
        params = list(params) if params is not None else list(getattr(flat, "module_order", None) or flat.params)
        for p in params:
            if id(p) not in flat.param_offset:
                raise ValueError("every optimized parameter must live in the flat buffer")
        # fused=None keeps torch from validating device support for the CPU path; the flag is
        # recorded in param_groups for state_dict parity with the reference.
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        for g in self.param_groups:
            g["fused"] = bool(fused)
        if len(self.param_groups) != 1:
            raise ValueError("FlatAdamW supports a single param group (the reference uses one)")
        self.flat = flat
        flat.layout_frozen = True  # the moments below are laid out like the flat buffers
        self.grad_scale = grad_scale  # e.g. 1/world_size after a SUM all-reduce
        self.grad_scale_dev: Optional[torch.Tensor] = None  # device-side multiplier (clipping)
        # fp32 master + fp32 moments for 16-bit parameters (fp32 / fp64 models already update in place)
        self.master: Optional[torch.Tensor] = None
        self._master_requested = bool(master_weights)
        if master_weights and flat.data.element_size() == 2:
            self.master = flat.data.float()
        sdt = torch.float32 if self.master is not None else flat.data.dtype
        self.exp_avg = torch.zeros(flat.data.shape, dtype=sdt, device=flat.data.device)
        self.exp_avg_sq = torch.zeros(flat.data.shape, dtype=sdt, device=flat.data.device)
        self._step = 0
        self._bind_state()
        self.overlap = False
        self._in_step = False
        self._done_ranges = []
        self._held = []  # (bucket, lo, hi, work) of reduced buckets not yet enqueued (OPT_SCHED "attn")
        self._gathers = []  # parameter all-gathers issued behind the updates (sharded optimizer)
        self._window_seen = False  # an attention window released held buckets (HIP attention path)
        self.pre_update_fences = []  # callables run on the update stream before any update
        # graph mode (train.py --compile): step-dependent scalars come from device memory
        self.graph_mode = False
        self.hyper: Optional[torch.Tensor] = None
        self._hyper_ring = []
        self._hyper_slot = 0
        self.guard: Optional[LossScaleGuard] = None  # --loss-scale: device-side skip / scale decisions
        # --stochastic-rounding: tensor mask (bit 0 p, 1 exp_avg, 2 exp_avg_sq; 0 = round to nearest), seed,
        # and the device copy of the step number a replayed graph reads (graph mode without a guard)
        self.sr_mask = 0
        self.sr_mode = "off"
        self.sr_seed = 0
        self.step_dev: Optional[torch.Tensor] = None

    # --- stochastic rounding ------------------------------------------------------------------
    def enable_stochastic_rounding(self, mode: str = "all", seed: int = 0):
        """Round the 16-bit state stochastically after every update: ``params`` the parameters only,
        ``all`` the parameters and both moments. An element's random bits depend only on ``seed``, the
        step number of the update (the one its bias corrections use), its position in the flat buffer
        and the tensor, so neither rank, bucket, stream, launch order nor graph replay changes them.
        The flat layout depends on the world size, so a resume at another world size draws other bits."""
        if mode not in _sr.MODES:
            raise ValueError(f"stochastic rounding mode must be one of {sorted(_sr.MODES)}, got {mode!r}")
        if self._master_requested or self.master is not None:
            raise ValueError("stochastic rounding rounds the pure 16-bit optimizer state; with master_weights=True "
                             "the state is fp32 and there is nothing to round: use one or the other")
        if self.flat.data.dtype not in (torch.bfloat16, torch.float16):
            raise ValueError(f"stochastic rounding needs bf16 or fp16 parameters; {self.flat.data.dtype} state is "
                             "not rounded after the update")
        seed = int(seed)
        if not 0 <= seed < 2 ** 64:
            raise ValueError(f"stochastic rounding seed must fit 64 unsigned bits, got {seed}")
        self.sr_mode, self.sr_mask, self.sr_seed = mode, _sr.MODES[mode], seed

    def _sr_kwargs(self, base: int) -> dict:
        """The SR launches' extra arguments for a slice that starts at flat position ``base``. Step
        number: the guard's applied count (device), the uploaded copy (graph mode), else the host's."""
        if self.guard is not None and self.guard.native:
            step_dev = self.guard.state[LossScaleGuard.APPLIED:LossScaleGuard.APPLIED + 1]
        else:
            step_dev = self.step_dev if self.graph_mode else None
        return {"seed": self.sr_seed, "base": int(base), "step": int(self._step), "step_dev": step_dev,
                "mask": self.sr_mask}

    # --- loss scale / non-finite step guard ---------------------------------------------------
    def enable_guard(self, guard: LossScaleGuard):
        """Every update takes its gradient multiplier, its skip flag and (GPU) its bias corrections from
        ``guard``, which the caller runs once per step between the backward and :meth:`step`
        (:meth:`LossScaleGuard.run`). The step count becomes the guard's applied count: it does not
        advance on a skipped step, and the host reads it only in :meth:`state_dict` / :meth:`applied_steps`.
        On the GPU the kernels always read ``hyper``; the host uploads only the learning rate."""
        self.guard = guard
        guard.betas = tuple(float(b) for b in self.param_groups[0]["betas"])
        guard.set_applied(self._step)
        self.grad_scale_dev = guard.multiplier
        guard.native = _ext.hip(self.flat.data)
        if guard.native:
            self._alloc_hyper()
            guard.hyper = self.hyper

    def applied_steps(self) -> int:
        """Updates applied so far (guard mode: read from the device, which synchronizes)."""
        if self.guard is not None:
            self._step = self.guard.read()["applied"]
        return self._step

    def _alloc_hyper(self):
        if self.hyper is None:
            self.hyper = torch.zeros(3, dtype=torch.float64, device=self.flat.data.device)
            self.step_dev = torch.zeros(1, dtype=torch.int32, device=self.flat.data.device)
            # pinned staging ring: a slot is rewritten only after its previous H2D copy completed
            self._hyper_ring = [(torch.zeros(3, dtype=torch.float64).pin_memory(),
                                 torch.zeros(1, dtype=torch.int32).pin_memory(), torch.cuda.Event())
                                for _ in range(4)]

    def _upload_hyper(self):
        """{lr, bc1, bc2_sqrt} -> ``hyper``; guard mode: lr only (the guard kernel writes the rest).
        Stochastic rounding without a guard: the step number -> ``step_dev`` as well."""
        lr, _, _, _, _, bc1, bc2_sqrt = self._coeffs()
        host, host_step, ev = self._hyper_ring[self._hyper_slot]
        self._hyper_slot = (self._hyper_slot + 1) % len(self._hyper_ring)
        ev.synchronize()
        host[0], host[1], host[2] = lr, bc1, bc2_sqrt
        n = 1 if self.guard is not None else 3
        self.hyper[:n].copy_(host[:n], non_blocking=True)
        if self.sr_mask and self.guard is None:
            host_step[0] = self._step
            self.step_dev.copy_(host_step, non_blocking=True)
        ev.record()

    # --- captured-step (HIP graph) support ---------------------------------------------------
    def enable_graph_mode(self):
        """Kernels read {lr, bc1, bc2_sqrt} from ``self.hyper`` (device fp64[3]) instead of
        launch arguments, and the host step counter advances in :meth:`begin_graph_step`, so one
        captured step replays correctly at every later step and learning rate."""
        if not self.flat.data.is_cuda:
            raise RuntimeError("graph mode needs the parameters on a GPU")
        self.graph_mode = True
        self._alloc_hyper()

    def begin_graph_step(self):
        """Host side of one replayed step: advance the step count and upload the scalars."""
        if self.guard is None:  # guard mode: the applied count lives on the device
            self._step += 1
        self._upload_hyper()

    # --- overlapped update (optimizer-in-backward) ----------------------------------------
    def enable_overlap(self, reducer):
        """Update each gradient bucket as soon as it is reduced, on a side stream, overlapped with
        the rest of the backward pass. Math and result are identical to :meth:`step`."""
        self.overlap = True
        self.reducer = reducer
        reducer.hooks.append(self._on_bucket)
        self.stream = torch.cuda.Stream(device=self.flat.data.device) if self.flat.data.is_cuda else None
        dev = self.flat.data.device
        sched.add_attention_window_hook(self.release_held, dev.index if dev.type == "cuda" else None)

    def _coeffs(self):
        g = self.param_groups[0]
        b1, b2 = g["betas"]
        lr, eps, wd = float(g["lr"]), float(g["eps"]), float(g["weight_decay"])
        return lr, b1, b2, eps, wd, 1.0 - b1 ** self._step, math.sqrt(1.0 - b2 ** self._step)

    def _update_range(self, lo, hi, coeffs=None):
        f = self.flat
        lr, b1, b2, eps, wd, bc1, bc2_sqrt = coeffs if coeffs is not None else self._coeffs()
        if not _ext.hip(f.data):
            self._step_reference(lr, b1, b2, eps, wd, bc1, bc2_sqrt, lo, hi)
            return
        C = _ext.require_for(f.data)
        # the last one is skip_dev: None is the kernels' unguarded path
        args = (lr, b1, b2, eps, wd, bc1, bc2_sqrt, self.grad_scale, self.grad_scale_dev, self.hyper, FAST_MATH,
                self.guard.skip_dev if self.guard is not None else None)
        m, v = self.exp_avg, self.exp_avg_sq
        sharded = self._sharded()
        if self.master is not None:
            # fp32 master update, then the transposed shadows of the matrices in range from the
            # rounded parameters (same stream: the next backward sees them; sharded: after the gather)
            C.adamw_master_(f.data[lo:hi], self.master[lo:hi], f.grad[lo:hi], m[lo:hi], v[lo:hi], *args)
            if not sharded:
                f.refresh_transposed(lo, hi)
            return
        # stochastic rounding: the same launches through the SR entry points, every slice with its flat
        # position, so the bits do not depend on how the range is cut
        flat_fn, t_fn = (C.adamw_flat_sr_, C.adamw_t_sr_) if self.sr_mask else (C.adamw_flat_, C.adamw_t_)
        sr = self._sr_kwargs if self.sr_mask else (lambda base: {})

        def update_flat(a, b):
            if a < b:
                flat_fn(f.data[a:b], f.grad[a:b], m[a:b], v[a:b], *args, **sr(a))

        def update_matrix(o, rows, cols):
            sl = slice(o, o + rows * cols)
            t_fn(f.data[sl].view(rows, cols), f.grad[sl].view(rows, cols), m[sl].view(rows, cols),
                 v[sl].view(rows, cols), f.data_t[sl].view(cols, rows), *args, **sr(o))

        if sharded:
            # an owned chunk cuts matrices: plain update; the shadows are re-derived from the gathered
            # parameters (step)
            update_flat(lo, hi)
            return
        cur, rest = lo, []
        for o, rows, cols in (f.transposed_in(lo, hi) if FUSED_T else []):
            if o + rows * cols > hi:  # (buckets align to fusion groups; kept for safety)
                rest.append(o)
                continue
            update_flat(cur, o)
            update_matrix(o, rows, cols)
            cur = o + rows * cols
        update_flat(cur, hi)
        if not FUSED_T:
            f.refresh_transposed(lo, hi)  # same stream: the next backward sees the new weights
        # A matrix that hi cuts was updated up to hi by the flat launches above; its shadow is re-derived
        # here from the whole matrix. That does not make the shadow right: the part beyond hi is updated by
        # a later range, and that range (the matrix starts before its lo) does not refresh the shadow again.
        for o in rest:
            f.refresh_transposed(o, o + 1)

    def _on_bucket(self, b, lo, hi, work):
        if not self.overlap or self.grad_scale_dev is not None:
            return  # clipping needs the global norm first: fall back to step()
        if not self._in_step:
            self._in_step = True
            if not self.graph_mode:  # graph mode: begin_graph_step() counts the step
                self._step += 1
        if self.stream is None:
            if work is not None:
                work.wait()
            self._update_bucket(b, lo, hi)
            return
        if self._held and not self._window_seen:
            # no attention window has released held buckets yet: this model's backward may offer
            # none, so do not wait any longer than one bucket
            self.release_held()
        self._held.append((b, lo, hi, work))
        if OPT_SCHED != "attn":
            self.release_held()

    def release_held(self, event=None):
        """Enqueue the held bucket updates on the side stream behind `event` (default: one recorded
        on the compute stream now). Every read of their weights was enqueued before the bucket was
        published, so any later point of the compute stream is safe."""
        if event is not None:
            self._window_seen = True  # called from an attention window of this device
        if not self._held:
            return
        if event is None:
            event = torch.cuda.Event()
            event.record()
        with torch.cuda.stream(self.stream):
            self.stream.wait_event(event)
            for b, lo, hi, work in self._held:
                if work is not None:
                    work.wait()  # update stream waits for the bucket's all-reduce
                for fence in self.pre_update_fences:
                    fence()
                self._update_bucket(b, lo, hi)
        self._held = []

    # --- sharded optimizer (GradReducer(shard=True), --shard-optimizer) ----------------------
    def _sharded(self) -> bool:
        r = getattr(self, "reducer", None) or getattr(self.flat, "reducer", None)
        return bool(r is not None and r.shard)

    def _update_bucket(self, b, lo, hi, coeffs=None):
        """Update bucket b's parameters this rank owns, then (sharded) all-gather them, issued on the
        current stream behind the update."""
        r = getattr(self.flat, "reducer", None)
        if r is None or not r.shard:
            self._update_range(lo, hi, coeffs)
            self._done_ranges.append((lo, hi))
            return
        for a, z in r.owned(b):
            self._update_range(a, z, coeffs)
            self._done_ranges.append((a, z))
        self._gathers.extend(r.gather_params(b))

    def _finish_gathers(self):
        """The current stream waits for the parameter all-gathers; the transposed shadows are then
        re-derived from the gathered parameters."""
        if not self._gathers and not self._sharded():
            return
        for w in self._gathers:
            w.wait()
        self._gathers = []
        r = getattr(self.flat, "reducer", None)
        if r is not None:
            r.gathers_done()  # xGMI engine: its step barrier goes behind the parameter gathers
        self.flat.refresh_transposed()

    def gather_state(self):
        """Collective (sharded optimizer): all-gather the moments (and the fp32 master) so every rank
        holds the full optimizer state, as a checkpoint stores it. A no-op otherwise."""
        r = getattr(self.flat, "reducer", None)
        if r is None or not r.shard:
            return
        if self.overlap and self.stream is not None:
            torch.cuda.current_stream(self.flat.data.device).wait_stream(self.stream)
        ts = [self.exp_avg, self.exp_avg_sq] + ([self.master] if self.master is not None else [])
        works = [w for b in range(r.num_buckets) for w in r.gather_params(b, ts)]
        for w in works:
            w.wait()

    def _bind_state(self):
        for p in self.param_groups[0]["params"]:
            o = self.flat.param_offset[id(p)]
            n = p.numel()
            self.state[p] = {
                "step": torch.tensor(float(self._step), dtype=torch.float32),
                "exp_avg": self.exp_avg[o:o + n].view(p.shape),
                "exp_avg_sq": self.exp_avg_sq[o:o + n].view(p.shape),
            }
            if self.master is not None:
                self.state[p]["master_param"] = self.master[o:o + n].view(p.shape)

    # --- torch.optim.Optimizer API ------------------------------------------------------
    def zero_grad(self, set_to_none: bool = True):
        """Marks gradient slots fresh; the flat gradient views are never set to None."""
        self.flat.zero_grad()
        if self.overlap and self.stream is not None:
            # the next backward overwrites gradients the update stream may still be reading
            torch.cuda.current_stream(self.flat.data.device).wait_stream(self.stream)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self.overlap and self.grad_scale_dev is None:
            self.reducer.finish()  # launches (and so updates) any bucket not yet ready
            if not self._in_step and not self.graph_mode:  # no bucket fired (no backward this step)
                self._step += 1
            self.release_held()
            if self.stream is not None:
                torch.cuda.current_stream(self.flat.data.device).wait_stream(self.stream)
            self._finish_gathers()
            self._in_step = False
            self._done_ranges = []
            return loss
        if self.guard is not None:
            # the guard ran on this step's gradient (LossScaleGuard.run). GPU: skip flag, multiplier and
            # bias corrections are in device memory; CPU: the applied count is read here
            if self.guard.native:
                if not self.graph_mode:
                    self._upload_hyper()
            else:
                self._step = int(self.guard.state[LossScaleGuard.APPLIED])
        elif not self.graph_mode:
            self._step += 1
        coeffs = self._coeffs()
        r = getattr(self.flat, "reducer", None)
        if r is not None and r.shard:
            for b, (lo, hi) in enumerate(r.ranges):
                self._update_bucket(b, lo, hi, coeffs)
            self._done_ranges = []
            self._finish_gathers()
            return loss
        self._update_range(0, self.flat.numel, coeffs)
        return loss

    def _step_reference(self, lr, b1, b2, eps, wd, bc1, bc2_sqrt, lo=0, hi=None):
        f = self.flat
        hi = f.numel if hi is None else hi
        if self.guard is not None and int(self.guard.state[LossScaleGuard.FOUND]):
            return  # skipped step: parameters, moments and the master stay as they are
        gs = self.grad_scale * (float(self.grad_scale_dev[0]) if self.grad_scale_dev is not None else 1.0)
        # `.data`: the update must not bump the flat buffer's autograd version counter (shared by
        # every parameter view), or an overlapped bucket update during backward would invalidate
        # weights other layers saved for their backward (the HIP kernels write through pointers)
        pd, gd, md, vd = f.data.data[lo:hi], f.grad[lo:hi], self.exp_avg[lo:hi], self.exp_avg_sq[lo:hi]
        ct = torch.promote_types(pd.dtype, torch.float32)  # fp32 opmath; fp64 models stay fp64
        p = (self.master[lo:hi] if self.master is not None else pd).to(ct)
        gr = gd.to(ct) * gs
        m = md.to(ct)
        v = vd.to(ct)
        p.mul_(1 - lr * wd)
        m.lerp_(gr, 1 - b1)
        v.mul_(b2).addcmul_(gr, gr, value=1 - b2)
        denom = v.sqrt().div_(bc2_sqrt).add_(eps)
        p.addcdiv_(m, denom, value=-(lr / bc1))
        if self.master is not None:
            self.master[lo:hi].copy_(p)
        if self.sr_mask:
            # the kernels' rounding rule with the kernels' bits (optim/sr.py): positions lo..hi-1
            idx = torch.arange(lo, hi, dtype=torch.int64, device=pd.device)
            for dst, val, stream in ((pd, p, _sr.STREAM_P), (md, m, _sr.STREAM_M), (vd, v, _sr.STREAM_V)):
                if self.sr_mask >> stream & 1:
                    val = _sr.stochastic_round(val, dst.dtype, idx, self._step, stream, self.sr_seed)
                dst.copy_(val)
            return
        pd.copy_(p)
        md.copy_(m)
        vd.copy_(v)

    # --- checkpoint compatibility -------------------------------------------------------
    def checkpoint_bytes(self) -> int:
        """Tensor bytes a checkpoint of this model + optimizer holds: the parameters, both moments
        and (``--master-weights fp32``) the fp32 master -- 6 B/param pure bf16, 14 B/param with the
        master. Sizes the time-aware final-save estimate and the pinned staging pool."""
        n = self.flat.data.nbytes + self.exp_avg.nbytes + self.exp_avg_sq.nbytes
        return n + (self.master.nbytes if self.master is not None else 0)

    def state_dict(self):
        self.applied_steps()  # guard mode: the applied count, from the device
        for st in self.state.values():
            st["step"] = torch.tensor(float(self._step), dtype=torch.float32)
        return super().state_dict()

    def load_state_dict(self, state_dict, tensors_loaded: bool = False):
        """Accepts torch.optim.AdamW state dicts (ours or the reference's). ``tensors_loaded``:
        the moments were already written into the flat buffers (native resume path), so only the
        hyper-parameters and step counts are taken from ``state_dict``."""
        groups = state_dict["param_groups"]
        if len(groups) != 1:
            raise ValueError("expected exactly one param group")
        params = self.param_groups[0]["params"]
        saved_ids = groups[0]["params"]
        if len(saved_ids) != len(params):
            raise ValueError(f"optimizer state has {len(saved_ids)} params, model has {len(params)}")
        for k, v in groups[0].items():
            if k != "params":
                self.param_groups[0][k] = v
        steps = set()
        with torch.no_grad():
            for sid, p in zip(saved_ids, params):
                st = state_dict["state"].get(sid, state_dict["state"].get(str(sid)))
                mine = self.state[p]
                if "master_param" in mine and (st is None or "master_param" not in st or not tensors_loaded):
                    # a checkpoint without a master (pure-bf16 run, the reference's): take the loaded
                    # parameters; with one, its fp32 values
                    src = st.get("master_param") if st is not None else None
                    mine["master_param"].copy_(src if src is not None else p.detach())
                if st is None:
                    if not tensors_loaded:
                        mine["exp_avg"].zero_()
                        mine["exp_avg_sq"].zero_()
                    continue
                if not tensors_loaded:
                    mine["exp_avg"].copy_(st["exp_avg"])
                    mine["exp_avg_sq"].copy_(st["exp_avg_sq"])
                steps.add(float(st["step"]))
        if len(steps) > 1:
            raise ValueError(f"inconsistent per-parameter step counts {sorted(steps)}")
        self._step = int(steps.pop()) if steps else 0
        if self.guard is not None:
            self.guard.set_applied(self._step)
        for st in self.state.values():
            st["step"] = torch.tensor(float(self._step), dtype=torch.float32)
