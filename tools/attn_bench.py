#!/usr/bin/env python
"""Attention kernel microbenchmark: forward / backward TFLOP/s of the HIP flash kernels on the
bench shape (default B=4, S=2048, Hq=Hkv=32, D=128, causal), on random data (rule: never on zeros).

FLOP convention (causal halves): fwd 4*B*H*S^2*D/2, bwd (dkdv + dq kernels, recompute included)
14*B*H*S^2*D/2 -- the work the kernels actually do -- and the "model" bwd convention 10*... .

--docs N [N ...]: also time the document-masked kernels (csrc/kernels/attention_docs.hip) with N equal
documents per row, next to the default causal kernels in the same process: the arms alternate over
--rounds rounds (each a warmed window of --iters calls) and the median per arm is printed, one JSON
line each, with the visible share of the causal area (1 / N) and the time relative to the causal arm.
"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4)
    ap.add_argument("--S", type=int, default=2048)
    ap.add_argument("--Hq", type=int, default=32)
    ap.add_argument("--Hkv", type=int, default=32)
    ap.add_argument("--D", type=int, default=128)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--noncausal", action="store_true")
    ap.add_argument("--docs", type=int, nargs="+", default=None,
                    help="equal documents per row for the document-masked kernels (S %% N == 0)")
    ap.add_argument("--rounds", type=int, default=5, help="alternating rounds per arm (--docs)")
    a = ap.parse_args()
    from pyrecover_amd import _ext

    C = _ext.native()
    dev = torch.device("cuda", 0)
    B, S, Hq, Hkv, D = a.B, a.S, a.Hq, a.Hkv, a.D
    causal = not a.noncausal
    torch.manual_seed(0)
    qkv = torch.randn(B * S, (Hq + 2 * Hkv) * D, device=dev).bfloat16()
    nq, nk = Hq * D, Hkv * D
    q = qkv[:, :nq].view(B, S, Hq, D)
    k = qkv[:, nq:nq + nk].view(B, S, Hkv, D)
    v = qkv[:, nq + nk:].view(B, S, Hkv, D)
    do = torch.randn(B, S, Hq, D, device=dev).bfloat16()
    dqkv = torch.empty_like(qkv)
    dq = dqkv[:, :nq].view(B, S, Hq, D)
    dk = dqkv[:, nq:nq + nk].view(B, S, Hkv, D)
    dv = dqkv[:, nq + nk:].view(B, S, Hkv, D)
    scale = 1 / math.sqrt(D)

    def fwd():
        return C.attn_fwd(q, k, v, scale, causal)

    o, lse = fwd()

    def bwd():
        C.attn_bwd(q, k, v, o, do, lse, dq, dk, dv, scale, causal)

    def timeit(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.iters

    if a.docs:
        import statistics

        if not causal or any(n <= 0 or S % n for n in a.docs):
            raise SystemExit("--docs: causal only, and S must be a multiple of every N")
        arms = {"causal": (fwd, bwd, o, lse)}
        for n in a.docs:
            ds = ((torch.arange(S, device=dev, dtype=torch.int32) // (S // n)) * (S // n)).repeat(B, 1).contiguous()
            on, ln = C.attn_fwd(q, k, v, scale, True, ds)
            arms[f"docs{n}"] = (lambda ds=ds: C.attn_fwd(q, k, v, scale, True, ds),
                                lambda ds=ds, on=on, ln=ln: C.attn_bwd(q, k, v, on, do, ln, dq, dk, dv, scale, True,
                                                                       None, 0, ds), on, ln)
        times = {name: ([], []) for name in arms}
        for r in range(a.rounds):
            names = list(arms) if r % 2 == 0 else list(arms)[::-1]
            for name in names:
                times[name][0].append(timeit(arms[name][0]))
                times[name][1].append(timeit(arms[name][1]))
        base_f, base_b = (statistics.median(t) for t in times["causal"])
        for name, (tfs, tbs) in times.items():
            mf, mb = statistics.median(tfs), statistics.median(tbs)
            n = 1 if name == "causal" else int(name[4:])
            rec = {"arm": name, "shape": dict(B=B, S=S, Hq=Hq, Hkv=Hkv, D=D), "visible_area": round(1 / n, 4),
                   "fwd_ms": round(mf, 4), "bwd_ms": round(mb, 4),
                   "fwd_min_max": [round(min(tfs), 4), round(max(tfs), 4)],
                   "bwd_min_max": [round(min(tbs), 4), round(max(tbs), 4)],
                   "fwd_vs_causal": round(mf / base_f, 3), "bwd_vs_causal": round(mb / base_b, 3)}
            print(json.dumps(rec), flush=True)
        return
    tf = timeit(fwd)
    tb = timeit(bwd)
    frac = 0.5 if causal else 1.0
    base = B * Hq * S * S * D * frac
    out = {"shape": dict(B=B, S=S, Hq=Hq, Hkv=Hkv, D=D, causal=causal), "fwd_ms": round(tf, 4),
           "bwd_ms": round(tb, 4), "fwd_tflops": round(4 * base / tf / 1e9, 1),
           "bwd_tflops_model": round(10 * base / tb / 1e9, 1), "bwd_tflops_executed": round(14 * base / tb / 1e9, 1)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
