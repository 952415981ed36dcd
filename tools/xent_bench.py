#!/usr/bin/env python
"""Fused cross-entropy kernels: the plain pair (xent_fwd + xent_bwd_) against the regularised pair
(xent_fwd_reg + xent_bwd_reg_: z-only, and z + label smoothing) in one process, arms alternating round
by round, timed with device events after a warm-up.

    python tools/xent_bench.py [--shapes 32768x32000,2048x128256,32768x128256] [--rounds 10] [--warmup 3]

The backward overwrites the logits, so every timed pair starts from a copy of the same bf16 logits (the
copy is outside the timed region). Bytes come from the shapes: the forward reads T*V*2, the backward reads
and writes it (3*T*V*2 for the pair). Prints one JSON line per shape and arm: median / min / max ms of the
pair, of its forward and its backward, the achieved GB/s of the pair, the difference from the plain pair
(median, %) and the plain pair's own run-to-run spread ((max - min) / median, %), which is the margin for
"costs the same".
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ARMS = (("plain", None), ("z", (1e-4, 0.0)), ("z+smooth", (1e-3, 0.1)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="32768x32000,2048x128256,32768x128256")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    from pyrecover_amd import _ext

    C = _ext.native()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    g = torch.ones(1, device=dev)
    for shape in a.shapes.split(","):
        T, V = (int(x) for x in shape.split("x"))
        gen = torch.Generator(device=dev)
        gen.manual_seed(T + V)
        master = (3 * torch.randn(T, V, device=dev, generator=gen)).to(torch.bfloat16)
        labels = torch.randint(0, V, (T,), device=dev, generator=gen)
        labels[::97] = -100
        work = torch.empty_like(master)

        def pair(coef):
            work.copy_(master)
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            e[0].record()
            if coef is None:
                lse, _, stats = C.xent_fwd(work, labels, -100)
                e[1].record()
                C.xent_bwd_(work, labels, lse, stats, g, -100)
            else:
                lse, stats = C.xent_fwd_reg(work, labels, -100, *coef)
                e[1].record()
                C.xent_bwd_reg_(work, labels, lse, stats, g, -100, *coef)
            e[2].record()
            return e

        for _ in range(a.warmup):
            for _, coef in ARMS:
                pair(coef)
        torch.cuda.synchronize()
        ev = {name: [] for name, _ in ARMS}
        for r in range(a.rounds):
            for name, coef in (ARMS if r % 2 == 0 else ARMS[::-1]):
                ev[name].append(pair(coef))
        torch.cuda.synchronize()
        ms = {n: [(e[0].elapsed_time(e[2]), e[0].elapsed_time(e[1]), e[1].elapsed_time(e[2])) for e in v]
              for n, v in ev.items()}
        base = statistics.median(t[0] for t in ms["plain"])
        spread = 100 * (max(t[0] for t in ms["plain"]) - min(t[0] for t in ms["plain"])) / base
        for name, _ in ARMS:
            tot, fwd, bwd = ([t[i] for t in ms[name]] for i in range(3))
            med = statistics.median(tot)
            print(json.dumps({"T": T, "V": V, "arm": name, "pair_ms": round(med, 4), "pair_min_ms": round(min(tot), 4),
                              "pair_max_ms": round(max(tot), 4), "fwd_ms": round(statistics.median(fwd), 4),
                              "bwd_ms": round(statistics.median(bwd), 4),
                              "pair_gb_per_s": round(3 * T * V * 2 / (med * 1e-3) / 1e9, 1),
                              "vs_plain_pct": round(100 * (med / base - 1), 2),
                              "plain_spread_pct": round(spread, 2)}), flush=True)
        del master, work


if __name__ == "__main__":
    main()
