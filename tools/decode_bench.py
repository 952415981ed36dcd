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
    python tools/decode_bench.py --extend 2048 --extend-base 0 --shapes 7b --batch 4 --ctx 2048   # ... beside docs_fwd
    python tools/decode_bench.py --prefill 4096 --prefill-chunk 0,512 --shapes 7b --batch 4 --layers 32

``--extend T`` times ``attn_extend`` (csrc/kernels/attention_extend.hip) alone: T new queries per sequence over
a cache that held ``--extend-base`` keys before (default ctx - T). ``--prefill S`` times ``prefill`` of a B x S
prompt once per ``--prefill-chunk`` value and prints the peak activation memory of each. ``--batch`` / ``--ctx``
override the shapes' batch and context.

``--kv-cache-dtype model|fp8|both`` picks the cache of every table: ``fp8`` is the e4m3fn cache with one
power-of-two scale per (token, kv head) (``attn_decode_fp8``; its K/V rate counts the bytes it reads, scales
included), ``both`` measures the two arms in one process on the same q and the same K / V values.

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
    n_buf = max(2, -(-2 * L3_BYTES // (per_layer8 if "fp8" in kinds else per_layer)))
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
    return hip, tor


def bench_extend(name, cfg, B, ctx, T, base, iters, dev):
    """``attn_extend`` alone: T new queries per sequence over a cache of capacity ctx that held ``base`` keys
    before the append (default ctx - T: the append fills the cache). With base 0 the call is a causal forward,
    and the document-masked forward (one document per row) is timed at the same shape beside it."""
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
    hip = timed_us(lambda i: C.attn_extend(q, ks[i % n_buf], vs[i % n_buf], n, scale), iters)
    o, _ = C.attn_extend(q, ks[0], vs[0], n, scale)
    blocks = -(-T * (Hq // Hkv) // 128) * Hkv * B
    print(f"{name}: attn_extend B={B} T={T} over kv_len={base} (cap {ctx}) Hq/Hkv={Hq}/{Hkv} D={D}: {blocks} blocks, "
          f"{per_layer / 2**20:.0f} MiB of K/V, {n_buf} caches in rotation")
    print(f"  HIP   {hip:9.1f} us  {flop / hip / 1e6:7.1f} TFLOP/s  {per_layer / hip / 1e6:6.2f} TB/s of K/V read once")
    if T * B * ctx <= 1 << 24:  # the oracle materialises [B, T, Hq, ctx] scores
        o_ref, _ = ref.attention_extend_ref(q.float(), ks[0].float(), vs[0].float(), n, scale)
        print(f"  max |o - o_ref| {(o.float() - o_ref).abs().max().item():.2e}")
    if base == 0 and T % 128 == 0:
        ds = torch.zeros(B, T, dtype=torch.int32, device=dev)
        kk, vv = [k[:, :T] for k in ks], [v[:, :T] for v in vs]
        docs = timed_us(lambda i: C.attn_fwd(q, kk[i % n_buf], vv[i % n_buf], scale, True, ds), iters)
        od, _ = C.attn_fwd(q, kk[0], vv[0], scale, True, ds)
        print(f"  docs_fwd, one document per row, same shape: {docs:9.1f} us  {flop / docs / 1e6:7.1f} TFLOP/s "
              f"(attn_extend takes {hip / docs:.2f}x; max |o - o_docs| {(o.float() - od.float()).abs().max().item():.2e})")
    return hip


def bench_prefill(name, preset, B, S, layers, chunks, iters, dev):
    """``prefill`` of a B x S prompt, one-shot (chunk 0) and in pieces: milliseconds and the peak of
    ``torch.cuda.max_memory_allocated`` above what the model and the cache hold."""
    cfg = get_preset(preset, n_layers=layers, seq_len=S)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    with torch.device(dev):
        model = Transformer(cfg)
    torch.set_default_dtype(prev)
    model.eval()
    model.flatten_(shadows=False)
    cache = inf.KVCache(cfg, B, S, torch.bfloat16, dev)
    tok = torch.randint(0, cfg.vocab_size, (B, S), device=dev)
    lens = torch.full((B,), S, device=dev)
    print(f"{name}: prefill of B={B} x S={S}, {layers} layers, bf16 (model + cache "
          f"{torch.cuda.memory_allocated() / 2**30:.2f} GiB resident)")
    first = None
    for c in chunks:
        inf.prefill(model, tok, lens, cache, chunk=c)  # library warm-up and GEMM tuning at this piece's shapes
        torch.cuda.synchronize()
        resident = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        us = timed_us(lambda _: inf.prefill(model, tok, lens, cache, chunk=c), iters, 1)
        peak = torch.cuda.max_memory_allocated() - resident
        logits = inf.prefill(model, tok, lens, cache, chunk=c).float()
        first = logits if first is None else first
        print(f"  chunk {c:5d}: prefill_ms {us / 1e3:9.2f}  peak activations {peak / 2**30:7.3f} GiB  "
              f"max |logits - logits(chunk {chunks[0]})| {(logits - first).abs().max().item():.3e}")


def filled_cache(cfg, B, ctx, dev, kv_dtype):
    """A full cache of standard normal K / V (quantized from them when fp8)."""
    cache = inf.KVCache(cfg, B, ctx, torch.bfloat16, dev, kv_dtype=kv_dtype)
    for i, (k, v) in enumerate(zip(cache.k, cache.v)):
        if cache.fp8:
            src = torch.randn(2, B, ctx, cfg.kv_heads, cfg.head_dim, device=dev).bfloat16()
            _ext.native().kv_quantize_(src[0], src[1], k, v, cache.k_scale[i], cache.v_scale[i])
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
    ap.add_argument("--kv-cache-dtype", choices=("model", "fp8", "both"), default="model",
                    help="the cache of every table: the model's dtype, fp8 (e4m3fn bytes + scales), or both arms")
    ap.add_argument("--extend", type=int, default=0, metavar="T",
                    help="time attn_extend alone: T new queries per sequence appended to each shape's cache")
    ap.add_argument("--extend-base", type=int, default=None, metavar="N",
                    help="keys the cache held before the append (default: ctx - T; 0 also times docs_fwd beside it)")
    ap.add_argument("--prefill", type=int, default=0, metavar="S",
                    help="time prefill of a B x S prompt, once per --prefill-chunk value, with its peak memory")
    ap.add_argument("--prefill-chunk", default="0,512", help="comma list of chunk sizes for --prefill (0: one-shot)")
    ap.add_argument("--batch", type=int, default=0, help="override the batch of every chosen shape")
    ap.add_argument("--ctx", type=int, default=0, help="override the context (cache capacity) of every chosen shape")
    a = ap.parse_args()
    shapes = [(s[0], s[1], a.batch or s[2], a.ctx or s[3]) for s in SHAPES if s[0] in a.shapes.split(",")]
    kinds = ("model", "fp8") if a.kv_cache_dtype == "both" else (a.kv_cache_dtype,)
    dev = torch.device("cuda", 0)
    _ext.native()
    if a.sample_bench:
        bench_sampler(a.iters, dev)
        return
    if a.extend:
        for name, preset, B, ctx in shapes:
            bench_extend(name, get_preset(preset), B, ctx, a.extend, a.extend_base, a.iters, dev)
        return
    if a.prefill:
        for name, preset, B, _ in shapes:
            bench_prefill(name, preset, B, a.prefill, a.layers, [int(c) for c in a.prefill_chunk.split(",")],
                          max(3, a.iters // 10), dev)
        return
    if a.sampler or a.graph:
        samplers = ("torch", "philox") if a.sampler == "both" else (a.sampler,) if a.sampler else ()
        for name, preset, B, ctx in shapes:
            for kind in kinds:
                bench_tokens(name, preset, B, ctx, a.layers, a.iters, dev, samplers, a.graph, kind)
        return
    for name, preset, B, ctx in shapes:
        bench_attention(name, get_preset(preset), B, ctx, a.iters, dev, kinds)
    if not a.skip_step:
        for name, preset, B, ctx in shapes:
            for kind in kinds:
                bench_step(name, preset, B, ctx, a.layers, max(10, a.iters // 2), dev, kind)


if __name__ == "__main__":
    main()
