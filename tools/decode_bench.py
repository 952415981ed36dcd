#!/usr/bin/env python
"""Decode-attention benchmark: ``attn_decode`` alone and a whole ``decode_step`` (tool, not a test).

Two shapes: the 7B shape (B 16, context 2048, MHA 32/32, head_dim 128) and the Llama-3-8B shape (B 1,
context 8192, GQA 32/8, head_dim 128). Prints microseconds and the achieved bytes/s of K/V read, next to
the same call through ``attention_decode_ref`` (torch math) on the GPU. The kernel streams K and V once,
so it is read against the achievable HBM streaming rate of MI355X (6.0-6.3 TB/s).

Every timed call reads another layer's cache (as a decode step does), and the layers together exceed the
256 MiB Infinity Cache, so the rate is an HBM rate and not a cache-hit rate.

    python tools/decode_bench.py [--layers 4] [--iters 50] [--skip-step] [--shapes 7b,llama3-8b]
    python tools/decode_bench.py --shapes 7b --sampler both --graph     # whole tokens: sample + bookkeeping + step
    python tools/decode_bench.py --sample-bench                         # the sampler alone
    python tools/decode_bench.py --kv-cache-dtype both                  # the fp8 cache beside the 16-bit one
    python tools/decode_bench.py --extend 8 --shapes llama3-8b          # attn_extend alone: 8 tokens onto a full cache
    python tools/decode_bench.py --extend 8 --extend-split 0 --shapes llama3-8b   # ... on the single pass (1: the key split)
    python tools/decode_bench.py --extend 2048 --extend-base 0 --shapes 7b --batch 4 --ctx 2048   # ... beside docs_fwd
    python tools/decode_bench.py --prefill 4096 --prefill-chunk 0,512 --shapes 7b --batch 4 --layers 32
    python tools/decode_bench.py --page-size 64,128,256 [--extend 8]    # the paged kernels beside the dense ones

``--extend T`` times ``attn_extend`` (csrc/kernels/attention_extend.hip) alone: T new queries per sequence over
a cache that held ``--extend-base`` keys before (default ctx - T). ``--prefill S`` times ``prefill`` of a B x S
prompt once per ``--prefill-chunk`` value and prints the peak activation memory of each. ``--batch`` / ``--ctx``
override the shapes' batch and context.

``--kv-cache-dtype model|fp8|both|fp4|all`` picks the cache of every table: ``fp8`` is the e4m3fn cache with one
power-of-two scale per (token, kv head) (``attn_decode_fp8``; its K/V rate counts the bytes it reads, scales
included), ``both`` measures the two arms in one process on the same q and the same K / V values. ``fp4`` is the
MXFP4 cache (``attn_decode_fp4``; e2m1 nibbles and one scale byte per 32 columns), timed beside the 16-bit call,
``all`` the three arms, alternating over three rounds.

``--sampler torch|philox|both`` times whole generated tokens (sampling, the bookkeeping of ``generate`` and the
decode step) per arm: ``torch`` is generate()'s default loop (``sample_token`` with a ``torch.Generator`` and
the out / count / done updates as torch ops), ``philox`` the one-launch ``DeviceSampler``; ``--graph`` adds the
philox arm replayed as a hipGraph (``DecodeGraph``). Temperature 0.8, top-k 50, top-p 0.95. One process per
shape keeps the arms on one allocator and one set of tuned GEMMs. ``--sample-bench`` times ``sample_`` against
``filter_logits`` + ``torch.multinomial`` on random bf16 logits (and on an all-equal row, the worst case for
histogram contention).

The times are device events around back-to-back calls: at batch 1 a call (two small kernels plus the
binding's allocations) can cost the host more than the kernels take, so read the kernels' own time from a
`rocprofv3 --kernel-trace --stats -- python tools/decode_bench.py --skip-step --shapes llama3-8b` run.
"""
import argparse
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from pyrecover_amd import _ext  # noqa: E402
from pyrecover_amd import inference as inf  # noqa: E402
from pyrecover_amd.config import get_preset  # noqa: E402
from pyrecover_amd.models.llama import Transformer  # noqa: E402
from pyrecover_amd.ops import reference as ref  # noqa: E402

SHAPES = [("7b", "llama2-7b", 16, 2048), ("llama3-8b", "llama3-8b", 1, 8192)]
L3_BYTES = 256 << 20


def timed_us(fn, iters, warmup=5):
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def bench_attention(name, cfg, B, ctx, iters, dev, kinds=("model",)):
    C = _ext.native()
    Hq, Hkv, D = cfg.n_heads, cfg.kv_heads, cfg.head_dim
    per_layer = 2 * B * ctx * Hkv * D * 2  # bytes of K and V one call reads
    per_layer8 = 2 * B * ctx * Hkv * (D + 4)  # ... from an fp8 cache: bytes and scales
    # rotate over >= 2 x the Infinity Cache (of the smaller arm's bytes)
    smallest = per_layer * (D // 2 + D // 32) // (2 * D) if "fp4" in kinds else per_layer8 if "fp8" in kinds else per_layer
    n_buf = max(2, -(-2 * L3_BYTES // smallest))
    ks = [torch.randn(B, ctx, Hkv, D, device=dev).bfloat16() for _ in range(n_buf)]
    vs = [torch.randn(B, ctx, Hkv, D, device=dev).bfloat16() for _ in range(n_buf)]
    q = torch.randn(B, Hq, D, device=dev).bfloat16()
    n = torch.full((B,), ctx, device=dev, dtype=torch.int32)
    scale = 1 / math.sqrt(D)
    hip8 = None
    if "fp8" in kinds:
        c8 = []
        for k, v in zip(ks, vs):
            kq, vq = torch.empty_like(k, dtype=torch.uint8), torch.empty_like(v, dtype=torch.uint8)
            sk, sv = (torch.empty(B, ctx, Hkv, device=dev) for _ in range(2))
            C.kv_quantize_(k, v, kq, vq, sk, sv)
            c8.append((kq, vq, sk, sv))
        hip8 = timed_us(lambda i: C.attn_decode_fp8(q, *c8[i % n_buf], n, scale), iters)
        o8, _ = C.attn_decode_fp8(q, *c8[0], n, scale)
        kd, vd = (ref.kv_dequantize_ref(c8[0][j], c8[0][j + 2]) for j in (0, 1))
        err8 = (o8.float() - ref.attention_decode_ref(q, kd, vd, n, scale)[0]).abs().max().item()
        del kd, vd
    if "model" not in kinds:
        print(f"{name}: attn_decode_fp8 B={B} ctx={ctx} Hq/Hkv={Hq}/{Hkv} D={D} KC={C.attn_decode_fp8_chunk()} "
              f"({per_layer8 / 2**20:.0f} MiB of K/V bytes and scales per call, {n_buf} caches in rotation)")
        print(f"  HIP fp8 {hip8:7.1f} us  {per_layer8 / hip8 / 1e6:6.2f} TB/s   (max |o - o_ref(dequantized)| {err8:.2e})")
        return hip8, None
    hip = timed_us(lambda i: C.attn_decode(q, ks[i % n_buf], vs[i % n_buf], n, scale), iters)
    tor = timed_us(lambda i: ref.attention_decode_ref(q, ks[i % n_buf], vs[i % n_buf], n, scale), max(5, iters // 5), 2)
    o, _ = C.attn_decode(q, ks[0], vs[0], n, scale)
    o_ref, _ = ref.attention_decode_ref(q, ks[0], vs[0], n, scale)
    err = (o.float() - o_ref).abs().max().item()
    print(f"{name}: attn_decode B={B} ctx={ctx} Hq/Hkv={Hq}/{Hkv} D={D} KC={C.attn_decode_chunk()} "
          f"({per_layer / 2**20:.0f} MiB of K/V per call, {n_buf} caches in rotation)")
    print(f"  HIP   {hip:9.1f} us  {per_layer / hip / 1e6:6.2f} TB/s")
    print(f"  torch {tor:9.1f} us  {per_layer / tor / 1e6:6.2f} TB/s   (HIP is {tor / hip:.1f}x; max |o - o_ref| {err:.2e})")
    if hip8 is not None:
        print(f"  HIP fp8 {hip8:7.1f} us  {per_layer8 / hip8 / 1e6:6.2f} TB/s of {per_layer8 / 2**20:.0f} MiB (bytes and scales; "
              f"KC={C.attn_decode_fp8_chunk()}): {hip / hip8:.2f}x of the 16-bit call; "
              f"max |o - o_ref(dequantized)| {err8:.2e}")
    if "fp4" in kinds:
        bench_attention_fp4(C, q, ks, vs, c8 if hip8 is not None else None, n, scale, iters, per_layer, per_layer8)
    return hip, tor


def bench_attention_fp4(C, q, ks, vs, c8, n, scale, iters, per_layer, per_layer8):
    """``attn_decode_fp4`` over the same K / V values, quantized to MXFP4, beside the 16-bit call (and the fp8 call
    when it was set up): the arms alternate over three rounds, every round's time is printed, the medians are
    compared. Its K/V rate counts nibbles and scale bytes."""
    B, ctx, Hkv, D = ks[0].shape
    per_layer4 = 2 * B * ctx * Hkv * (D // 2 + D // 32)
    c4 = []
    for k, v in zip(ks, vs):
        kq, vq = (torch.empty(B, ctx, Hkv, D // 2, dtype=torch.uint8, device=q.device) for _ in range(2))
        sk, sv = (torch.empty(B, ctx, Hkv, D // 32, dtype=torch.uint8, device=q.device) for _ in range(2))
        C.kv_quantize_fp4_(k, v, kq, vq, sk, sv)
        c4.append((kq, vq, sk, sv))
    nb = len(ks)
    arms = [("16-bit", per_layer, lambda i: C.attn_decode(q, ks[i % nb], vs[i % nb], n, scale))]
    if c8 is not None:
        arms.append(("fp8", per_layer8, lambda i: C.attn_decode_fp8(q, *c8[i % nb], n, scale)))
    arms.append(("fp4", per_layer4, lambda i: C.attn_decode_fp4(q, *c4[i % nb], n, scale)))
    times = {a: [] for a, _, _ in arms}
    for _ in range(3):
        for a, _, fn in arms:
            times[a].append(timed_us(fn, iters))
    o4, _ = C.attn_decode_fp4(q, *c4[0], n, scale)
    kd, vd = (ref.kv_dequantize_fp4_ref(c4[0][j], c4[0][j + 2]) for j in (0, 1))
    err4 = (o4.float() - ref.attention_decode_ref(q, kd, vd, n, scale)[0]).abs().max().item()
    print(f"  fp4 beside the others, KC={C.attn_decode_fp4_chunk()}, us (three rounds, median); "
          f"max |o - o_ref(dequantized)| {err4:.2e}")
    med16 = sorted(times["16-bit"])[1]
    for a, nbytes, _ in arms:
        med = sorted(times[a])[1]
        print(f"  {a:7s} {med:8.1f} ({' '.join(f'{x:.1f}' for x in times[a])})  {nbytes / med / 1e6:5.2f} TB/s of "
              f"{nbytes / 2**20:.0f} MiB  {med16 / med:.2f}x of the 16-bit call")


def bench_extend(name, cfg, B, ctx, T, base, iters, dev, split=-1, kinds=("model",)):
    """``attn_extend`` alone: T new queries per sequence over a cache of capacity ctx that held ``base`` keys
    before the append (default ctx - T: the append fills the cache). With base 0 the call is a causal forward,
    and the document-masked forward (one document per row) is timed at the same shape beside it. ``split``:
    -1 by plan, 0 the single pass, 1 the key split. With "fp8" in ``kinds`` the same caches, quantized, are timed
    through ``attn_extend_fp8`` in the same process (same plan, same rotation), with "fp4" through
    ``attn_extend_fp4``. With more than one arm (fp8, fp4, docs_fwd) the arms alternate over three rounds; every round's time is printed, the median is the headline."""
    C = _ext.native()
    Hq, Hkv, D = cfg.n_heads, cfg.kv_heads, cfg.head_dim
    base = ctx - T if base is None else base
    if T < 1 or base < 0 or base + T > ctx:
        raise SystemExit(f"--extend: need 1 <= T and 0 <= base and base + T <= ctx, got T={T} base={base} ctx={ctx}")
    per_layer = 2 * B * (base + T) * Hkv * D * 2  # bytes of K and V the keys of one call hold
    n_buf = max(2, -(-2 * L3_BYTES // per_layer))
    ks = [torch.randn(B, ctx, Hkv, D, device=dev).bfloat16() for _ in range(n_buf)]
    vs = [torch.randn(B, ctx, Hkv, D, device=dev).bfloat16() for _ in range(n_buf)]
    q = torch.randn(B, T, Hq, D, device=dev).bfloat16()
    n = torch.full((B,), base, device=dev, dtype=torch.int32)
    scale = 1 / math.sqrt(D)
    flop = 4.0 * B * Hq * D * sum(base + t + 1 for t in range(T))  # q.k and p.v over the visible keys
    # Arms of one shape alternate inside a round and the round repeats (3 rounds when there is more than one
    # arm): the first timing of a process runs slow, and a later arm otherwise inherits a warmer machine.
    arms = [("16", lambda i: C.attn_extend(q, ks[i % n_buf], vs[i % n_buf], n, scale, split))]
    c8 = []
    if "fp8" in kinds:
        for k, v in zip(ks, vs):
            kq, vq = torch.empty_like(k, dtype=torch.uint8), torch.empty_like(v, dtype=torch.uint8)
            sk, sv = (torch.empty(B, ctx, Hkv, device=dev) for _ in range(2))
            C.kv_quantize_(k, v, kq, vq, sk, sv)
            c8.append((kq, vq, sk, sv))
        arms.append(("fp8", lambda i: C.attn_extend_fp8(q, *c8[i % n_buf], n, scale, split)))
    c4 = []
    if "fp4" in kinds:
        for k, v in zip(ks, vs):
            kq, vq = (torch.empty(B, ctx, Hkv, D // 2, dtype=torch.uint8, device=dev) for _ in range(2))
            sk, sv = (torch.empty(B, ctx, Hkv, D // 32, dtype=torch.uint8, device=dev) for _ in range(2))
            C.kv_quantize_fp4_(k, v, kq, vq, sk, sv)
            c4.append((kq, vq, sk, sv))
        arms.append(("fp4", lambda i: C.attn_extend_fp4(q, *c4[i % n_buf], n, scale, split)))
    with_docs = base == 0 and T % 128 == 0
    if with_docs:
        ds = torch.zeros(B, T, dtype=torch.int32, device=dev)
        kk, vv = [k[:, :T] for k in ks], [v[:, :T] for v in vs]
        arms.append(("docs", lambda i: C.attn_fwd(q, kk[i % n_buf], vv[i % n_buf], scale, True, ds)))
    rounds = 3 if len(arms) > 1 else 1
    times = {a: [] for a, _ in arms}
    for _ in range(rounds):
        for a, fn in arms:
            times[a].append(timed_us(fn, iters))
    med = {a: sorted(t)[len(t) // 2] for a, t in times.items()}
    every = {a: " ".join(f"{x:.1f}" for x in t) for a, t in times.items()}
    hip = med["16"]
    o, _ = C.attn_extend(q, ks[0], vs[0], n, scale, split)
    on = C.attn_extend_plan(B, T, Hq, Hkv, D, ctx)["split"] if split < 0 else bool(split)
    R, XC = T * (Hq // Hkv), C.attn_extend_chunk()
    waves = (4 if R <= 32 else 2 if R <= 64 else 1) if on else 1  # waves that share a 32-row sub-tile
    blocks = -(-R * waves // 128) * Hkv * B * (-(-ctx // XC) if on else 1)
    arm = f"key split, XC={XC}, {waves} waves per sub-tile" if on else "single pass"
    print(f"{name}: attn_extend B={B} T={T} over kv_len={base} (cap {ctx}) Hq/Hkv={Hq}/{Hkv} D={D}: "
          f"{'plan: ' if split < 0 else ''}{arm}, {blocks} blocks, "
          f"{per_layer / 2**20:.0f} MiB of K/V, {n_buf} caches in rotation")
    print(f"  HIP   {hip:9.1f} us  {flop / hip / 1e6:7.1f} TFLOP/s  {per_layer / hip / 1e6:6.2f} TB/s of K/V read once"
          + (f"  (median of rounds: {every['16']})" if rounds > 1 else ""))
    if T * B * ctx <= 1 << 24:  # the oracle materialises [B, T, Hq, ctx] scores
        o_ref, _ = ref.attention_extend_ref(q.float(), ks[0].float(), vs[0].float(), n, scale)
        print(f"  max |o - o_ref| {(o.float() - o_ref).abs().max().item():.2e}")
    if c8:
        per8, hip8 = per_layer // 2 // D * (D + 4), med["fp8"]
        print(f"  HIP fp8 {hip8:7.1f} us  {flop / hip8 / 1e6:7.1f} TFLOP/s  {per8 / hip8 / 1e6:6.2f} TB/s of "
              f"{per8 / 2**20:.0f} MiB (bytes and scales): {hip / hip8:.2f}x of the 16-bit call  "
              f"(median of rounds: {every['fp8']})")
        if T * B * ctx <= 1 << 24:
            o8, _ = C.attn_extend_fp8(q, *c8[0], n, scale, split)
            kd, vd = (ref.kv_dequantize_ref(c8[0][j], c8[0][j + 2]) for j in (0, 1))
            o_ref, _ = ref.attention_extend_ref(q.float(), kd, vd, n, scale)
            print(f"  max |o - o_ref(dequantized)| {(o8.float() - o_ref).abs().max().item():.2e}")
    if c4:
        per4, hip4 = per_layer // (2 * D) * (D // 2 + D // 32), med["fp4"]
        print(f"  HIP fp4 {hip4:7.1f} us  {flop / hip4 / 1e6:7.1f} TFLOP/s  {per4 / hip4 / 1e6:6.2f} TB/s of "
              f"{per4 / 2**20:.0f} MiB (nibbles and scales): {hip / hip4:.2f}x of the 16-bit call  "
              f"(median of rounds: {every['fp4']})")
        if T * B * ctx <= 1 << 24:
            o4, _ = C.attn_extend_fp4(q, *c4[0], n, scale, split)
            kd, vd = (ref.kv_dequantize_fp4_ref(c4[0][j], c4[0][j + 2]) for j in (0, 1))
            o_ref, _ = ref.attention_extend_ref(q.float(), kd, vd, n, scale)
            print(f"  max |o - o_ref(dequantized)| {(o4.float() - o_ref).abs().max().item():.2e}")
    if with_docs:
        docs = med["docs"]
        od, _ = C.attn_fwd(q, kk[0], vv[0], scale, True, ds)
        print(f"  docs_fwd, one document per row, same shape: {docs:9.1f} us  {flop / docs / 1e6:7.1f} TFLOP/s "
              f"(attn_extend takes {hip / docs:.2f}x; max |o - o_docs| {(o.float() - od.float()).abs().max().item():.2e}"
              f"; rounds: {every['docs']})")
    return hip


def bench_paged(name, cfg, B, ctx, pages, T, base, iters, dev, split=-1):
    """The paged kernels (csrc/kernels/attention_paged.hip) beside the dense ones on the same logical contents:
    ``attn_decode_paged`` over ctx keys (T = 0) or ``attn_extend_paged`` with T queries over ``base`` keys. Every
    page size's pool holds the dense caches' pages in a shuffled order. The arms alternate over three rounds;
    every round's time is printed, the medians are compared, and the outputs must be bit-equal."""
    C = _ext.native()
    Hq, Hkv, D = cfg.n_heads, cfg.kv_heads, cfg.head_dim
    base = (ctx - T if base is None else base) if T else ctx
    per_layer = 2 * B * (base + T) * Hkv * D * 2
    n_buf = max(2, -(-2 * L3_BYTES // per_layer))
    ks = [torch.randn(B, ctx, Hkv, D, device=dev).bfloat16() for _ in range(n_buf)]
    vs = [torch.randn(B, ctx, Hkv, D, device=dev).bfloat16() for _ in range(n_buf)]
    q = torch.randn(B, max(T, 1), Hq, D, device=dev).bfloat16()
    n = torch.full((B,), base, device=dev, dtype=torch.int32)
    scale = 1 / math.sqrt(D)
    if T:
        dense = lambda i: C.attn_extend(q, ks[i % n_buf], vs[i % n_buf], n, scale, split)  # noqa: E731
    else:
        dense = lambda i: C.attn_decode(q[:, 0], ks[i % n_buf], vs[i % n_buf], n, scale)  # noqa: E731
    what = f"attn_extend T={T} over kv_len={base}, split {split}" if T else "attn_decode"
    print(f"{name}: {what}, B={B} cap={ctx} Hq/Hkv={Hq}/{Hkv} D={D}, {per_layer / 2**20:.0f} MiB of K/V, "
          f"{n_buf} caches in rotation; dense vs paged, us (three rounds, median)")
    for page in pages:
        P = -(-ctx // page)
        perm = torch.randperm(B * P, generator=torch.Generator().manual_seed(page)).to(dev)
        bt = torch.empty(B * P, dtype=torch.int32, device=dev)
        bt[perm] = torch.arange(B * P, dtype=torch.int32, device=dev)  # pool page j holds dense page perm[j]
        bt = bt.view(B, P)

        def pool(x):
            pad = torch.zeros(B, P * page, Hkv, D, dtype=x.dtype, device=dev)
            pad[:, :ctx] = x
            return pad.view(B * P, page, Hkv, D)[perm].contiguous()

        kps, vps = [pool(k) for k in ks], [pool(v) for v in vs]
        if T:
            paged = lambda i: C.attn_extend_paged(q, kps[i % n_buf], vps[i % n_buf], bt, n, ctx, scale, split)  # noqa: E731
        else:
            paged = lambda i: C.attn_decode_paged(q[:, 0], kps[i % n_buf], vps[i % n_buf], bt, n, ctx, scale)  # noqa: E731
        td, tp = [], []
        for _ in range(3):
            td.append(timed_us(dense, iters))
            tp.append(timed_us(paged, iters))
        same = all(torch.equal(a, b) for a, b in zip(dense(0), paged(0)))
        md, mp = sorted(td)[1], sorted(tp)[1]
        print(f"  page {page:3d}: dense {md:8.1f} ({' '.join(f'{x:.1f}' for x in td)})  paged {mp:8.1f} "
              f"({' '.join(f'{x:.1f}' for x in tp)})  paged / dense {mp / md:.3f}  {per_layer / mp / 1e6:5.2f} TB/s  "
              f"bit-equal: {same}")
        del kps, vps


def bench_shared(name, cfg, G, ctx, page, N, iters, dev):
    """``attn_decode_shared_paged`` (csrc/kernels/attention_decode_shared.hip) beside ``attn_decode_paged`` on the same
    pools and table: G groups of N sequences of ctx keys whose first ctx - page keys are shared pages, the last
    page each sequence's own, pages shuffled. The arms alternate over three rounds; every round's time is printed
    and the medians compared. The bytes are those the pools hold (shared pages once) and those the per-sequence
    kernel streams (shared pages N times)."""
    C = _ext.native()
    Hq, Hkv, D = cfg.n_heads, cfg.kv_heads, cfg.head_dim
    P, B = ctx // page, G * N
    if ctx % page or P < 2:
        raise SystemExit(f"--shared: --ctx {ctx} must be at least two whole pages of {page}")
    npg = G * (P - 1 + N)
    once, streamed = 2 * npg * page * Hkv * D * 2, 2 * B * ctx * Hkv * D * 2
    n_buf = max(2, -(-2 * L3_BYTES // once))
    ids = torch.randperm(npg, generator=torch.Generator().manual_seed(page)).to(torch.int32)
    bt = torch.empty(G, N, P, dtype=torch.int32)
    bt[:, :, :P - 1] = ids[:G * (P - 1)].view(G, 1, P - 1)
    bt[:, :, P - 1] = ids[G * (P - 1):].view(G, N)
    bt = bt.view(B, P).to(dev)
    kps = [torch.randn(npg, page, Hkv, D, device=dev).bfloat16() for _ in range(n_buf)]
    vps = [torch.randn(npg, page, Hkv, D, device=dev).bfloat16() for _ in range(n_buf)]
    q = torch.randn(B, Hq, D, device=dev).bfloat16()
    n = torch.full((B,), ctx, device=dev, dtype=torch.int32)
    sl = torch.full((G,), ctx - page, device=dev, dtype=torch.int32)
    scale = 1 / math.sqrt(D)
    each = lambda i: C.attn_decode_paged(q, kps[i % n_buf], vps[i % n_buf], bt, n, ctx, scale)  # noqa: E731
    shared = lambda i: C.attn_decode_shared_paged(q, kps[i % n_buf], vps[i % n_buf], bt, n, sl, N, ctx, scale)  # noqa: E731
    te, ts = [], []
    for _ in range(3):
        te.append(timed_us(each, iters))
        ts.append(timed_us(shared, iters))
    err = max((a.float() - b.float()).abs().max().item() for a, b in zip(each(0), shared(0)))
    me, ms = sorted(te)[1], sorted(ts)[1]
    print(f"{name}: attn_decode, {G} groups of {N} x {ctx} keys ({ctx - page} shared), page {page}, Hq/Hkv={Hq}/{Hkv} "
          f"D={D}; pools {once / 2**20:.0f} MiB, streamed per sequence {streamed / 2**20:.0f} MiB, {n_buf} pools in "
          f"rotation; us (three rounds, median)")
    print(f"  per sequence {me:8.1f} ({' '.join(f'{x:.1f}' for x in te)})  {streamed / me / 1e6:5.2f} TB/s streamed   "
          f"shared {ms:8.1f} ({' '.join(f'{x:.1f}' for x in ts)})  {once / ms / 1e6:5.2f} TB/s of the pools   "
          f"shared / per sequence {ms / me:.3f}   max |difference| of o, lse {err:.2e}")


def bench_prefill(name, preset, B, S, layers, chunks, iters, dev, kv_dtype="model"):
    """``prefill`` of a B x S prompt, one-shot (chunk 0) and in pieces: milliseconds and the peak of
    ``torch.cuda.max_memory_allocated`` above what the model and the cache hold. An fp8 cache takes the pieces
    with ``fp8_extend=True``, an fp4 cache with ``fp4_extend=True``."""
    cfg = get_preset(preset, n_layers=layers, seq_len=S)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    with torch.device(dev):
        model = Transformer(cfg)
    torch.set_default_dtype(prev)
    model.eval()
    model.flatten_(shadows=False)
    cache = inf.KVCache(cfg, B, S, torch.bfloat16, dev, kv_dtype=kv_dtype)
    tok = torch.randint(0, cfg.vocab_size, (B, S), device=dev)
    lens = torch.full((B,), S, device=dev)
    print(f"{name}: prefill of B={B} x S={S}, {layers} layers, bf16, {kv_dtype} cache (model + cache "
          f"{torch.cuda.memory_allocated() / 2**30:.2f} GiB resident)")
    first = None
    opt = dict(fp8_extend=True, fp4_extend=True)
    for c in chunks:
        inf.prefill(model, tok, lens, cache, chunk=c, **opt)  # library warm-up and GEMM tuning at this piece's shapes
        torch.cuda.synchronize()
        resident = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        us = timed_us(lambda _: inf.prefill(model, tok, lens, cache, chunk=c, **opt), iters, 1)
        peak = torch.cuda.max_memory_allocated() - resident
        logits = inf.prefill(model, tok, lens, cache, chunk=c, **opt).float()
        first = logits if first is None else first
        print(f"  chunk {c:5d}: prefill_ms {us / 1e3:9.2f}  peak activations {peak / 2**30:7.3f} GiB  "
              f"max |logits - logits(chunk {chunks[0]})| {(logits - first).abs().max().item():.3e}")


def filled_cache(cfg, B, ctx, dev, kv_dtype):
    """A full cache of standard normal K / V (quantized from them when fp8 or fp4)."""
    cache = inf.KVCache(cfg, B, ctx, torch.bfloat16, dev, kv_dtype=kv_dtype)
    for i, (k, v) in enumerate(zip(cache.k, cache.v)):
        if cache.fp8 or cache.fp4:
            src = torch.randn(2, B, ctx, cfg.kv_heads, cfg.head_dim, device=dev).bfloat16()
            C = _ext.native()
            (C.kv_quantize_fp4_ if cache.fp4 else C.kv_quantize_)(src[0], src[1], k, v, cache.k_scale[i], cache.v_scale[i])
        else:
            k.normal_()
            v.normal_()
    return cache


def bench_step(name, preset, B, ctx, layers, iters, dev, kv_dtype="model"):
    cfg = get_preset(preset, n_layers=layers, seq_len=ctx)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    with torch.device(dev):
        model = Transformer(cfg)
    torch.set_default_dtype(prev)
    model.eval()
    model.flatten_(shadows=False)
    cache = filled_cache(cfg, B, ctx, dev, kv_dtype)
    tok = torch.randint(0, cfg.vocab_size, (B,), device=dev)

    def step(_):
        cache.kv_len.fill_(ctx - 1)  # the step appends row ctx - 1 and attends to all ctx keys
        inf.decode_step(model, tok, cache)

    us = timed_us(step, iters)
    kv = cache.nbytes()
    print(f"{name}: decode_step, {kv_dtype} cache ({kv / 2**20:.0f} MiB), {layers} layers, B={B} ctx={ctx}: "
          f"{us:9.1f} us ({us / layers:.1f} us per layer; "
          f"K/V read {kv / us / 1e6:.2f} TB/s of step time)")
    return us


SAMPLING = dict(temperature=0.8, top_k=50, top_p=0.95)


def bench_tokens(name, preset, B, ctx, layers, iters, dev, samplers, graph, kv_dtype="model"):
    cfg = get_preset(preset, n_layers=layers, seq_len=ctx)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    with torch.device(dev):
        model = Transformer(cfg)
    torch.set_default_dtype(prev)
    model.eval()
    model.flatten_(shadows=False)
    cache = filled_cache(cfg, B, ctx, dev, kv_dtype)
    warmup = 8
    total = warmup + iters
    start = ctx - total - 2  # the timed tokens end on a nearly full cache and never fill it
    lens = torch.full((B,), start, dtype=torch.long, device=dev)
    room = torch.full((B,), ctx, dtype=torch.long, device=dev)
    tok0 = torch.randint(0, cfg.vocab_size, (B,), device=dev)
    results = {}

    def fresh_logits():
        cache.kv_len.fill_(start)
        return inf.decode_step(model, tok0, cache)

    if "torch" in samplers:
        gen = torch.Generator(device=dev)
        gen.manual_seed(0)
        st = {"logits": fresh_logits(), "done": torch.zeros(B, dtype=torch.bool, device=dev),
              "out": torch.full((B, total), -1, dtype=torch.long, device=dev),
              "count": torch.zeros(B, dtype=torch.long, device=dev), "i": 0}

        def step_torch(_):  # the statements of generate()'s default loop
            i = st["i"]
            tok = inf.sample_token(st["logits"], generator=gen, **SAMPLING)
            st["out"][:, i] = torch.where(st["done"], st["out"][:, i], tok)
            st["count"] += (~st["done"]).long()
            st["done"] = st["done"] | (room <= i)
            tok = torch.where(st["done"], torch.zeros_like(tok), tok)
            st["logits"] = inf.decode_step(model, tok, cache)
            st["i"] = i + 1

        results["eager + torch"] = timed_us(step_torch, iters, warmup)
    if "philox" in samplers:
        ds = inf.DeviceSampler(lens, room, total, seed=0, **SAMPLING)
        st2 = {"logits": fresh_logits()}

        def step_philox(_):
            st2["logits"] = inf.decode_step(model, ds.sample(st2["logits"]), cache)

        results["eager + philox"] = timed_us(step_philox, iters, warmup)
    if graph:
        ds = inf.DeviceSampler(lens, room, total, seed=0, **SAMPLING)
        dg = inf.DecodeGraph(model, cache, fresh_logits(), ds)
        results["graph + philox"] = timed_us(lambda _: dg.step(), iters, warmup)
        assert dg.captured
    print(f"{name}: one generated token (sample + bookkeeping + decode_step), {kv_dtype} cache, {layers} layers, B={B} "
          f"ctx={ctx}, V={cfg.vocab_size}")
    base = results.get("eager + torch")
    for arm, us in results.items():
        rel = f"  ({base / us:.2f}x of eager + torch)" if base and arm != "eager + torch" else ""
        print(f"  {arm:15s} {us:9.1f} us per token, {us / layers:7.1f} us per layer{rel}")
    return results


def bench_sampler(iters, dev):
    C = _ext.native()
    print("sampler alone, bf16 logits, T 0.8: us per call")
    print(f"  {'V':>7s} {'B':>3s} {'setting':>10s} {'input':>9s} {'sample_':>9s} {'torch':>9s}")
    for V in (32000, 128256):
        for B in (1, 16):
            pos = torch.arange(B, device=dev, dtype=torch.int32)
            tok = torch.empty(B, dtype=torch.long, device=dev)
            ws = torch.empty(C.sample_ws_bytes(B) // 4, dtype=torch.int32, device=dev)
            gen = torch.Generator(device=dev)
            gen.manual_seed(0)
            inputs = [("normal", (torch.randn(B, V, device=dev) * 3).bfloat16()),
                      ("all-equal", torch.full((B, V), 1.5, device=dev).bfloat16())]
            for setting, k, p in (("top-k 50", 50, 1.0), ("top-p 0.95", 0, 0.95)):
                for kind, x in inputs:
                    hip = timed_us(lambda i: C.sample_(x, tok, 0.8, k, p, 0, pos=pos, ws=ws), iters)
                    tor = timed_us(lambda i: inf.sample_token(x, 0.8, k, p, gen), max(5, iters // 5), 2)
                    print(f"  {V:7d} {B:3d} {setting:>10s} {kind:>9s} {hip:9.1f} {tor:9.1f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=4, help="layers of the model the decode_step timing builds")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--shapes", default="7b,llama3-8b", help="comma list of: 7b, llama3-8b")
    ap.add_argument("--sampler", choices=("torch", "philox", "both"), default=None,
                    help="time whole generated tokens with this sampler instead of the kernel / step tables")
    ap.add_argument("--graph", action="store_true", help="add the hipGraph-replayed philox arm (DecodeGraph)")
    ap.add_argument("--sample-bench", action="store_true", help="time the sampler alone")
    ap.add_argument("--kv-cache-dtype", choices=("model", "fp8", "both", "fp4", "all"), default="model",
                    help="the cache of every table: the model's dtype, fp8 (e4m3fn bytes + scales), both of them, fp4 "
                         "(MXFP4 nibbles + block scales; the kernel table times it beside the 16-bit call), or all "
                         "three arms. fp4 has no paged kernel: --page-size and --shared refuse it")
    ap.add_argument("--extend", type=int, default=0, metavar="T",
                    help="time attn_extend alone: T new queries per sequence appended to each shape's cache")
    ap.add_argument("--extend-base", type=int, default=None, metavar="N",
                    help="keys the cache held before the append (default: ctx - T; 0 also times docs_fwd beside it)")
    ap.add_argument("--extend-split", choices=("auto", "0", "1"), default="auto",
                    help="--extend: the kernel by plan (auto), the single pass (0) or the key split (1)")
    ap.add_argument("--page-size", default="", metavar="64,128,256",
                    help="time the paged kernels against the dense ones on the same contents, pages shuffled: "
                         "attn_decode_paged, or with --extend T attn_extend_paged")
    ap.add_argument("--shared", type=int, default=0, metavar="N",
                    help="time attn_decode_shared_paged beside attn_decode_paged: the shape's batch as groups of N "
                         "sequences over a common prefix of --ctx minus one page (--page-size, default 128)")
    ap.add_argument("--prefill", type=int, default=0, metavar="S",
                    help="time prefill of a B x S prompt, once per --prefill-chunk value, with its peak memory")
    ap.add_argument("--prefill-chunk", default="0,512", help="comma list of chunk sizes for --prefill (0: one-shot)")
    ap.add_argument("--batch", type=int, default=0, help="override the batch of every chosen shape")
    ap.add_argument("--ctx", type=int, default=0, help="override the context (cache capacity) of every chosen shape")
    a = ap.parse_args()
    shapes = [(s[0], s[1], a.batch or s[2], a.ctx or s[3]) for s in SHAPES if s[0] in a.shapes.split(",")]
    kinds = {"both": ("model", "fp8"), "all": ("model", "fp8", "fp4")}.get(a.kv_cache_dtype, (a.kv_cache_dtype,))
    if "fp4" in kinds and (a.page_size or a.shared):
        raise SystemExit("--kv-cache-dtype fp4 / all: there is no paged fp4 kernel, so --page-size and --shared take "
                         "model, fp8 or both")
    dev = torch.device("cuda", 0)
    _ext.native()
    if a.sample_bench:
        bench_sampler(a.iters, dev)
        return
    if a.shared:
        for name, preset, B, ctx in shapes:
            for page in [int(p) for p in (a.page_size or "128").split(",")]:
                bench_shared(name, get_preset(preset), B, ctx, page, a.shared, a.iters, dev)
        return
    if a.page_size:
        for name, preset, B, ctx in shapes:
            bench_paged(name, get_preset(preset), B, ctx, [int(p) for p in a.page_size.split(",")], a.extend,
                        a.extend_base, a.iters, dev, -1 if a.extend_split == "auto" else int(a.extend_split))
        return
    if a.extend:
        for name, preset, B, ctx in shapes:
            bench_extend(name, get_preset(preset), B, ctx, a.extend, a.extend_base, a.iters, dev,
                         -1 if a.extend_split == "auto" else int(a.extend_split), kinds)
        return
    if a.prefill:
        for name, preset, B, _ in shapes:
            for kind in kinds:
                bench_prefill(name, preset, B, a.prefill, a.layers, [int(c) for c in a.prefill_chunk.split(",")],
                              max(3, a.iters // 10), dev, kind)
        return
    if a.sampler or a.graph:
        samplers = ("torch", "philox") if a.sampler == "both" else (a.sampler,) if a.sampler else ()
        for name, preset, B, ctx in shapes:
            for kind in kinds:
                bench_tokens(name, preset, B, ctx, a.layers, a.iters, dev, samplers, a.graph, kind)
        return
    for name, preset, B, ctx in shapes:
        bench_attention(name, get_preset(preset), B, ctx, a.iters, dev,
                        kinds if "fp4" not in kinds else tuple(dict.fromkeys(("model",) + kinds)))
    if not a.skip_step:
        for name, preset, B, ctx in shapes:
            for kind in kinds:
                bench_step(name, preset, B, ctx, a.layers, max(10, a.iters // 2), dev, kind)


if __name__ == "__main__":
    main()
