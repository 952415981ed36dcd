"""KV-cache generation: prefill, single-token decode steps and sampling from a :class:`Transformer`.

Nothing here touches the training paths. ``prefill`` runs the ops of the training forward (embedding,
fused add + norm, fused QKV GEMM, RoPE, the causal ``attn_fwd``, W1|W3 + SwiGLU, W2) with identical
rounding points, keeps every layer's rotated k and plain v in a :class:`KVCache` and applies the final
norm and the output GEMM to the last prompt row of each sequence only. ``decode_step`` pushes one token
per sequence through all layers on the two kernels of csrc/kernels/attention_decode.hip:
``rope_append`` (rotate q in place, write rotated k / plain v into the cache row ``kv_len[b]``) and
``attn_decode`` (one query per sequence over the cache). ``kv_len`` lives on the device and no kernel
argument depends on a host copy of it: a decode step never synchronises.

``extend`` appends T > 1 tokens per sequence to a cache that already holds keys (a follow-up turn, a
continuation after a shared prefix, a scoring or verification pass): the T-token ``rope_append`` and
``attn_extend`` of csrc/kernels/attention_extend.hip (T queries per sequence over keys 0 .. kv_len[b] + t).
A short append over a long cache runs its key-split arm (attention_extend_split.hip: fixed key chunks, fp32
partials, an ordered combine) by a plan that reads shapes and the CU count only; see :func:`attention_extend`.
``prefill(chunk=N)`` feeds a prompt through it in pieces of N columns, so the prefill's activation memory
is bounded by the piece. Both refuse an fp8 cache unless ``fp8_extend=True``: then the new tokens are
quantized into the cache first and every query attends to dequantized rows, as in ``decode_step``
(csrc/kernels/attention_extend_fp8.hip, the T-token ``rope_append_fp8``).

The HIP decode kernels take bf16 / fp16 at head_dim 64 / 128. CPU tensors, fp32 / fp64 models on the
GPU and other head dims run the torch math of :mod:`pyrecover_amd.ops.reference`
(``attention_decode_ref`` / ``attention_extend_ref`` / ``rope_append_ref``), noted once through
``_note_fallback`` like attention.

``KVCache(kv_dtype="fp8")`` (``generate(kv_cache_dtype="fp8")``) keeps k / v as OCP e4m3fn bytes with one
power-of-two scale per (token, kv head), about half the cache's memory and half the bytes a decode step
reads: csrc/kernels/attention_decode_fp8.hip (``kv_quantize``, ``rope_append_fp8``, ``attn_decode_fp8``), the
rule in ``ops/reference.py::kv_quantize_ref``. The prompt's attention stays unquantized; only what is stored
is quantized. Opt-in: without it nothing changes.

``KVCache(kv_dtype="fp4")`` (``generate(kv_cache_dtype="fp4")``) keeps k / v as OCP MXFP4: e2m1 nibbles with one
power-of-two e8m0 scale per block of 32 columns, D / 2 + D / 32 bytes per head row, about half the fp8 cache:
csrc/kernels/attention_decode_fp4.hip (``kv_quantize_fp4``, ``rope_append_fp4``, ``attn_decode_fp4``), the rule in
``ops/reference.py::kv_quantize_fp4_ref``. As with fp8 the prompt's attention stays unquantized. ``extend`` and the
chunked prefill refuse it unless ``fp4_extend=True``, which serves it as ``fp8_extend=True`` serves an fp8 cache: the
T-token ``rope_append_fp4``, then ``attn_extend_fp4`` (csrc/kernels/attention_extend_fp4.hip) over the dequantized
rows.

:class:`PagedKVCache` (``generate(kv_page_size=N)``) keeps k / v in a pool of pages of 64, 128 or 256 tokens with
one block table per batch: a sequence pays for the pages it reserved instead of ``capacity`` rows, and a shared
prefix is shared pages (:meth:`PagedKVCache.share_prefix`). ``prefill``, ``extend``, the chunked prefill,
``decode_step`` and :class:`DecodeGraph` take either cache; with a paged one the four cache ops run the page-walking
kernels of csrc/kernels/attention_paged.hip, which return the dense kernels' bits. Opt-in: the default is dense.

Sampling has two rules. ``sampler="torch"`` (the default) filters with ``torch.topk`` / ``torch.sort`` and
draws with ``torch.multinomial`` from a seeded ``torch.Generator``. ``sampler="philox"`` is the stateless
rule of csrc/kernels/sample.hip (:func:`sample_philox`): the uniform of a draw is a Philox function of
(seed, row, absolute position), so tokens do not depend on how many were drawn before, and the kernel
also keeps ``out`` / ``count`` / ``done`` on the device (:class:`DeviceSampler`). With it nothing in a
token's work depends on the host, and :class:`DecodeGraph` replays sample -> ``decode_step`` as one
hipGraph (``generate(graph=True)``).
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _ext
from .config import TransformerModelArgs
from .ops import fused as F
from .ops import reference as ref

SYNC_EVERY = 16  # generate(): the finished mask is read back at most once per this many tokens


KV_DTYPES = ("model", "fp8", "fp4")


class KVCache:
    """Per-layer k / v of shape [B, capacity, Hkv, D] (token-major, like every activation here) and the
    int32 device tensor ``kv_len`` [B] of tokens held per sequence.

    ``kv_dtype="model"`` (the default) stores k / v in ``dtype``. ``kv_dtype="fp8"`` stores every head row
    as D bytes of OCP e4m3fn (uint8 tensors ``k`` / ``v``) and one power-of-two fp32 scale (``k_scale`` /
    ``v_scale`` [B, capacity, Hkv]) by the rule of ``ops/reference.py::kv_quantize_ref``: (D + 4) / (2 D)
    of the 16-bit cache's bytes. ``kv_dtype="fp4"`` stores it as OCP MXFP4 by the rule of
    ``ops/reference.py::kv_quantize_fp4_ref``: uint8 ``k`` / ``v`` [B, capacity, Hkv, D / 2] of e2m1 nibble pairs
    and uint8 ``k_scale`` / ``v_scale`` [B, capacity, Hkv, D / 32] of e8m0 exponents, one per block of 32 columns:
    (D / 2 + D / 32) / (2 D) of the 16-bit cache's bytes; head_dim must be a multiple of 32. ``dtype`` stays the
    model's dtype: the dtype of q and of the output."""

    def __init__(self, model_args: TransformerModelArgs, batch: int, capacity: int, dtype: torch.dtype, device,
                 kv_dtype: str = "model"):
        if kv_dtype not in KV_DTYPES:
            raise ValueError(f"KVCache: kv_dtype must be one of {KV_DTYPES}, got {kv_dtype!r}")
        if capacity > model_args.seq_len:
            raise ValueError(f"KVCache capacity {capacity} exceeds the model's seq_len {model_args.seq_len} "
                             f"(the extent of the RoPE table)")
        if batch < 1 or capacity < 1:
            raise ValueError(f"KVCache needs batch >= 1 and capacity >= 1, got {batch}, {capacity}")
        self.batch, self.capacity, self.dtype, self.kv_dtype = batch, capacity, dtype, kv_dtype
        self.fp8, self.fp4 = kv_dtype == "fp8", kv_dtype == "fp4"
        D = model_args.head_dim
        if self.fp4 and D % 32:
            raise ValueError(f"KVCache: kv_dtype='fp4' needs head_dim a multiple of 32 (the MX block), got {D}")
        shape = (model_args.n_layers, batch, capacity, model_args.kv_heads, D // 2 if self.fp4 else D)
        self._k = torch.zeros(shape, dtype=torch.uint8 if self.fp8 or self.fp4 else dtype, device=device)
        self._v = torch.zeros_like(self._k)
        self.k = list(self._k.unbind(0))
        self.v = list(self._v.unbind(0))
        n = model_args.n_layers
        self.k_scale, self.v_scale = [None] * n, [None] * n
        if self.fp8:  # an all-zero row has scale 1
            self._k_scale = torch.ones(shape[:-1], dtype=torch.float32, device=device)
            self._v_scale = torch.ones_like(self._k_scale)
            self.k_scale = list(self._k_scale.unbind(0))
            self.v_scale = list(self._v_scale.unbind(0))
        if self.fp4:  # an all-zero block has e = 0: byte 127
            self._k_scale = torch.full(shape[:-1] + (D // 32,), 127, dtype=torch.uint8, device=device)
            self._v_scale = torch.full_like(self._k_scale, 127)
            self.k_scale = list(self._k_scale.unbind(0))
            self.v_scale = list(self._v_scale.unbind(0))
        self.kv_len = torch.zeros(batch, dtype=torch.int32, device=device)

    def nbytes(self) -> int:
        n = 2 * self._k.numel() * self._k.element_size()
        if self.fp8 or self.fp4:
            n += 2 * self._k_scale.numel() * self._k_scale.element_size()
        return n


PAGE_SIZES = (64, 128, 256)  # divide the decode chunk (256) and the extend chunk (512); multiples of the 64-key tile


class PagedKVCache:
    """A KV cache in pages: per layer ``k[i]`` / ``v[i]`` are pools [n_pages, page_size, Hkv, D] and one int32
    ``block_table`` [B, ceil(capacity / page_size)] on the device (shared by all layers, -1: unmapped) maps the
    logical position j of sequence b to row ``j % page_size`` of page ``block_table[b, j // page_size]``
    (csrc/kernels/attention_paged.hip). ``capacity`` is the logical capacity, with :class:`KVCache`'s meaning
    and rule; ``kv_len`` is the same int32 device tensor. A sequence pays for the pages it reserved, not for
    ``capacity`` rows, and two sequences may name the same page (:meth:`share_prefix`).

    The allocator lives on the host: a free list and a reference count per page. :meth:`reserve` /
    :meth:`release` / :meth:`share_prefix` push a changed table row with one small host-to-device copy; call
    them outside a captured region and before a decode loop, never inside one (``generate`` reserves every
    sequence's pages before the prefill, so the table is static while decoding). ``n_pages`` defaults to
    ``batch * ceil(capacity / page_size)``, the dense cache's footprint. A paged fp8 cache is a follow-up.

    :meth:`fork` turns every sequence into ``group_size`` consecutive rows that share its pages. A forked cache
    carries ``shared_len`` (int32 [batch / group_size] on the device, with a host mirror): the leading tokens of a
    group whose table entries are the same in every member's row. ``decode_step`` hands both to
    ``attn_decode_shared_paged``, which reads those pages once per group. :meth:`release` and
    :meth:`share_prefix` keep it truthful (they only ever lower it); :meth:`reserve` maps pages after a row's
    mapped prefix and cannot break it."""

    fp8 = fp4 = False
    kv_dtype = "model"
    group_size = 1      # > 1 after fork(): rows g * group_size .. (g + 1) * group_size - 1 form group g
    shared_len = None   # forked: int32 [batch / group_size] on the device

    def __init__(self, model_args: TransformerModelArgs, batch: int, capacity: int, dtype: torch.dtype, device,
                 page_size: int = 128, n_pages: Optional[int] = None, kv_dtype: str = "model"):
        if kv_dtype == "fp4":
            raise ValueError("PagedKVCache: kv_dtype='fp4' is not served: a paged fp4 cache is a follow-up")
        if kv_dtype != "model":
            raise ValueError(f"PagedKVCache: kv_dtype={kv_dtype!r} is not served: a paged fp8 cache is a follow-up")
        if page_size not in PAGE_SIZES:
            raise ValueError(f"PagedKVCache: page_size must be one of {PAGE_SIZES}, got {page_size}")
        if capacity > model_args.seq_len:
            raise ValueError(f"PagedKVCache capacity {capacity} exceeds the model's seq_len {model_args.seq_len} "
                             f"(the extent of the RoPE table)")
        if batch < 1 or capacity < 1:
            raise ValueError(f"PagedKVCache needs batch >= 1 and capacity >= 1, got {batch}, {capacity}")
        self.batch, self.capacity, self.dtype, self.page_size = batch, capacity, dtype, page_size
        self.pages_per_seq = -(-capacity // page_size)
        self.n_pages = batch * self.pages_per_seq if n_pages is None else int(n_pages)
        if self.n_pages < 1:
            raise ValueError(f"PagedKVCache needs n_pages >= 1, got {n_pages}")
        shape = (model_args.n_layers, self.n_pages, page_size, model_args.kv_heads, model_args.head_dim)
        self._k = torch.zeros(shape, dtype=dtype, device=device)
        self._v = torch.zeros_like(self._k)
        self.k = list(self._k.unbind(0))
        self.v = list(self._v.unbind(0))
        self.k_scale, self.v_scale = [None] * model_args.n_layers, [None] * model_args.n_layers
        self.kv_len = torch.zeros(batch, dtype=torch.int32, device=device)
        self.block_table = torch.full((batch, self.pages_per_seq), -1, dtype=torch.int32, device=device)
        self._free = list(range(self.n_pages - 1, -1, -1))  # pop() hands out ascending ids
        self._refs = [0] * self.n_pages
        self._pages: List[List[int]] = [[] for _ in range(batch)]  # the mapped prefix of each table row

    def _push(self, b: int) -> None:
        row = self._pages[b] + [-1] * (self.pages_per_seq - len(self._pages[b]))
        self.block_table[b].copy_(torch.tensor(row, dtype=torch.int32))

    def _take(self, n: int, what: str) -> List[int]:
        if n > len(self._free):
            raise RuntimeError(f"PagedKVCache: {what} needs {n} more page(s) of {self.page_size} tokens, the pool of "
                               f"{self.n_pages} has {len(self._free)} free: short by {n - len(self._free)}")
        got = [self._free.pop() for _ in range(n)]
        for p in got:
            self._refs[p] = 1
        return got

    def reserve(self, b: int, n_tokens: int) -> None:
        """Map pages so that sequence ``b`` can hold ``n_tokens`` (<= capacity). Idempotent, grows only."""
        if not 0 <= n_tokens <= self.capacity:
            raise ValueError(f"PagedKVCache.reserve: n_tokens must be in 0 .. {self.capacity}, got {n_tokens}")
        more = -(-n_tokens // self.page_size) - len(self._pages[b])
        if more <= 0:
            return
        self._pages[b] += self._take(more, f"reserve({b}, {n_tokens})")
        self._push(b)

    def release(self, b: int) -> None:
        """Unmap sequence ``b`` (``kv_len[b]`` = 0); pages nobody else names go back to the free list."""
        for p in self._pages[b]:
            self._refs[p] -= 1
            if self._refs[p] == 0:
                self._free.append(p)
        self._pages[b] = []
        self._push(b)
        self.kv_len[b] = 0
        self._set_shared(b // self.group_size, 0)  # its row agrees with nobody's any more

    def _set_shared(self, g: int, n_tokens: int) -> None:
        if self.group_size > 1 and n_tokens != self._shared[g]:
            self._shared[g] = n_tokens
            self.shared_len[g] = n_tokens

    def share_prefix(self, src: int, dst: int, n_tokens: int) -> None:
        """Sequence ``dst`` (released first) becomes a copy of the first ``n_tokens`` (a host int, at most what
        ``src`` holds) of ``src``: it names ``src``'s first ``n_tokens // page_size`` pages, gets a fresh page with a
        device copy of the partial page if there is one, and ``kv_len[dst] = n_tokens``. Whatever ``dst`` appends
        from there on lands on pages it owns alone. On a forked cache ``dst``'s group keeps the part of its
        ``shared_len`` that the new row still agrees with when ``src`` is a member of it, and none otherwise."""
        full, rem = divmod(int(n_tokens), self.page_size)
        if src == dst or n_tokens < 0 or full + (rem > 0) > len(self._pages[src]):
            raise ValueError(f"PagedKVCache.share_prefix: sequence {src} has no {n_tokens} tokens mapped to share "
                             f"with {dst}")
        g = dst // self.group_size
        keep = 0
        if self.group_size > 1 and src // self.group_size == g:  # the others agree with src on _shared[g] tokens
            keep = min(self._shared[g], full * self.page_size)
        self.release(dst)  # shared_len[g] = 0 until the new row stands
        own = self._take(1, f"share_prefix({src}, {dst}, {n_tokens})") if rem else []
        shared = self._pages[src][:full]
        for p in shared:
            self._refs[p] += 1
        if rem:
            s = self._pages[src][full]
            self._k[:, own[0], :rem].copy_(self._k[:, s, :rem])
            self._v[:, own[0], :rem].copy_(self._v[:, s, :rem])
        self._pages[dst] = shared + own
        self._push(dst)
        self.kv_len[dst] = int(n_tokens)
        self._set_shared(g, keep)

    def fork(self, n: int, kv_len: Optional[Sequence[int]] = None) -> "PagedKVCache":
        """A cache of batch ``batch * n`` over the same pools and allocator state, for n samples per sequence; this
        object must not be used afterwards. New row ``g * n`` takes over old row g's pages; rows ``g * n + 1 ..
        g * n + n - 1`` are :meth:`share_prefix` copies of it at its current length: the full pages are named
        again, a partial page is copied into a fresh page per copy. ``group_size = n`` and ``shared_len[g] =
        (kv_len_g // page_size) * page_size``. ``kv_len``: the host's knowledge of the lengths (``generate`` passes
        the prompt lengths); without it ``self.kv_len`` is read back once. A pool without ``(n - 1)`` free pages
        for every partial page raises the allocator's "short by" error and changes nothing."""
        if n < 1 or self.group_size != 1:
            raise ValueError(f"PagedKVCache.fork: n must be >= 1 on a cache that is not forked yet, got {n}")
        lens = [int(x) for x in (self.kv_len.tolist() if kv_len is None else kv_len)]
        ps, B = self.page_size, self.batch
        if len(lens) != B or any(L < 0 or -(-L // ps) > len(self._pages[b]) for b, L in enumerate(lens)):
            raise ValueError(f"PagedKVCache.fork: kv_len must hold {B} lengths inside the mapped pages, got {lens}")
        own = self._take((n - 1) * sum(L % ps > 0 for L in lens), f"fork({n})")
        new = object.__new__(PagedKVCache)
        new.__dict__.update(self.__dict__)  # the pools, the free list and the reference counts are shared
        new.batch, new.group_size = B * n, n
        new._pages, new._shared = [], []
        for g, L in enumerate(lens):
            full, rem = divmod(L, ps)
            src = self._pages[g]
            new._pages.append(src)
            for p in src[:full]:
                self._refs[p] += n - 1
            mine = [own.pop() for _ in range(n - 1)] if rem else []
            if mine:  # one broadcast copy of the partial page per pool
                self._k[:, mine, :rem] = self._k[:, src[full]:src[full] + 1, :rem]
                self._v[:, mine, :rem] = self._v[:, src[full]:src[full] + 1, :rem]
            new._pages += [src[:full] + [p] for p in mine] if rem else [src[:full] for _ in range(n - 1)]
            new._shared.append(full * ps)
        dev = self.kv_len.device
        rows = [r + [-1] * (self.pages_per_seq - len(r)) for r in new._pages]
        new.block_table = torch.tensor(rows, dtype=torch.int32).to(dev)
        new.kv_len = torch.tensor([L for L in lens for _ in range(n)], dtype=torch.int32).to(dev)
        new.shared_len = torch.tensor(new._shared, dtype=torch.int32).to(dev)
        return new

    def pages_in_use(self) -> int:
        return self.n_pages - len(self._free)

    def nbytes(self) -> int:
        """Bytes of the pools and the table (what the cache allocates, whatever is mapped)."""
        return 2 * self._k.numel() * self._k.element_size() + self.block_table.numel() * 4


def _paged_kw(cache) -> Dict:
    """The keyword arguments that make the cache ops below walk pages: none for a dense cache."""
    if isinstance(cache, PagedKVCache):
        return {"block_table": cache.block_table, "cap": cache.capacity}
    return {}


def _group_kw(cache) -> Dict:
    """The further keyword arguments of :func:`attention_decode` over a forked :class:`PagedKVCache`."""
    if getattr(cache, "group_size", 1) > 1:
        return {"group_size": cache.group_size, "shared_len": cache.shared_len}
    return {}


def _decode_hip(qkv: torch.Tensor, head_dim: int) -> bool:
    return F._note_fallback("decode attention", qkv, _ext.hip16(qkv) and head_dim in (64, 128))


def _scale_kind(k_scale) -> Tuple[bool, bool]:
    """(fp8, fp4) from a cache op's ``k_scale``: fp32 scales mark an fp8 cache, uint8 e8m0 bytes an fp4 cache."""
    fp4 = k_scale is not None and k_scale.dtype == torch.uint8
    return k_scale is not None and not fp4, fp4


def rope_append(qkv, tab, kv_len, k_cache, v_cache, k_scale=None, v_scale=None, block_table=None, cap=None) -> None:
    """The new tokens' fused QKV rows [B * T, (Hq + 2 Hkv) D], T per sequence (B is the caches'): row
    b * T + t has q rotated in place at position kv_len[b] + t, rotated k and plain v into that cache row.
    Bit-equal to ``rope_`` on the same row at that position. T = 1 clamps the row to cap - 1; with T > 1 a
    position at or beyond the capacity stores nothing (its q takes table row cap - 1).
    With ``k_scale`` / ``v_scale`` the caches are fp8 (uint8): the same rows, for any T, are quantized on
    the way in -- the cache is a pure function of what the 16-bit cache would hold. uint8 scales mark an fp4
    cache (:class:`KVCache`): the same, by the MXFP4 rule.
    With ``block_table`` (and the logical capacity ``cap``) the caches are the pools of a :class:`PagedKVCache`: the
    same rows through the table, bit for bit; a token whose page is unmapped stores nothing."""
    fp8, fp4 = _scale_kind(k_scale)
    D = k_cache.shape[-1] * (2 if fp4 else 1)
    if block_table is not None:
        if _decode_hip(qkv, k_cache.shape[-1]):
            _ext.require_for(qkv).rope_append_paged_(qkv, tab, kv_len, k_cache, v_cache, block_table, cap)
        else:
            ref.rope_append_paged_ref(qkv, tab, kv_len, k_cache, v_cache, block_table, cap)
    elif _decode_hip(qkv, D):
        C = _ext.require_for(qkv)
        if fp4:
            C.rope_append_fp4_(qkv, tab, kv_len, k_cache, v_cache, k_scale, v_scale)
        elif fp8:
            C.rope_append_fp8_(qkv, tab, kv_len, k_cache, v_cache, k_scale, v_scale)
        else:
            C.rope_append_(qkv, tab, kv_len, k_cache, v_cache)
    elif fp4:
        ref.rope_append_fp4_ref(qkv, tab, kv_len, k_cache, v_cache, k_scale, v_scale)
    elif fp8:
        ref.rope_append_fp8_ref(qkv, tab, kv_len, k_cache, v_cache, k_scale, v_scale)
    else:
        ref.rope_append_ref(qkv, tab, kv_len, k_cache, v_cache)


def attention_decode(q, k_cache, v_cache, kv_len, scale: Optional[float] = None, k_scale=None,
                     v_scale=None, block_table=None, cap=None, group_size: int = 1,
                     shared_len=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """q [B, Hq, D] over the caches [B, cap, Hkv, D]: sequence b attends to keys 0 .. kv_len[b] - 1.
    Returns (o [B, Hq, D] in q's dtype, lse fp32 [B, Hq] -- the opmath dtype on the torch path).
    With ``k_scale`` / ``v_scale`` the caches are fp8 (uint8; fp4 when the scales are uint8 too) and the keys are
    their dequantized rows.
    With ``block_table`` / ``cap`` they are the pools of a :class:`PagedKVCache`: ``attn_decode_paged``, bit-equal
    to the dense kernel on the gathered cache. With ``group_size`` > 1 and ``shared_len`` (int32
    [B / group_size] on the device; a forked cache's fields) as well, the batch is groups of ``group_size``
    consecutive sequences whose table rows agree on ``shared_len[g]`` leading tokens: ``attn_decode_shared_paged``
    (csrc/kernels/attention_decode_shared.hip) reads those pages once per group. The result is the ungrouped one
    up to fp32 summation order (``ops/reference.py::attention_decode_shared_ref``)."""
    scale = scale if scale is not None else 1.0 / math.sqrt(q.shape[-1])
    fp8, fp4 = _scale_kind(k_scale)
    if group_size != 1 and (block_table is None or shared_len is None):
        raise ValueError("attention_decode: group_size > 1 needs a paged cache (block_table, cap) and shared_len")
    if block_table is not None:
        if _decode_hip(q, q.shape[-1]):
            C = _ext.require_for(q)
            if group_size != 1:
                o, lse = C.attn_decode_shared_paged(q, k_cache, v_cache, block_table, kv_len, shared_len, group_size,
                                                    cap, scale)
            else:
                o, lse = C.attn_decode_paged(q, k_cache, v_cache, block_table, kv_len, cap, scale)
            return o, lse
        o, lse = ref.attention_decode_shared_ref(q, k_cache, v_cache, block_table, kv_len, cap, scale, group_size,
                                                 shared_len)
        return o.to(q.dtype), lse
    if _decode_hip(q, q.shape[-1]):
        C = _ext.require_for(q)
        if fp4:
            o, lse = C.attn_decode_fp4(q, k_cache, v_cache, k_scale, v_scale, kv_len, scale)
        elif fp8:
            o, lse = C.attn_decode_fp8(q, k_cache, v_cache, k_scale, v_scale, kv_len, scale)
        else:
            o, lse = C.attn_decode(q, k_cache, v_cache, kv_len, scale)
        return o, lse
    if fp4:
        o, lse = ref.attention_decode_fp4_ref(q, k_cache, v_cache, k_scale, v_scale, kv_len, scale)
    elif fp8:
        o, lse = ref.attention_decode_fp8_ref(q, k_cache, v_cache, k_scale, v_scale, kv_len, scale)
    else:
        o, lse = ref.attention_decode_ref(q, k_cache, v_cache, kv_len, scale)
    return o.to(q.dtype), lse


def attention_extend(q, k_cache, v_cache, kv_len, scale: Optional[float] = None, split: Optional[bool] = None,
                     k_scale=None, v_scale=None, block_table=None, cap=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """q [B, T, Hq, D] over the caches [B, cap, Hkv, D], which hold the T new tokens' k / v already
    (:func:`rope_append` first); ``kv_len`` [B] counts the tokens held before the append. Query t of
    sequence b attends to keys 0 .. min(kv_len[b] + t, cap - 1). Returns (o [B, T, Hq, D] in q's dtype,
    lse fp32 [B, T, Hq] -- the opmath dtype on the torch path).

    ``split`` picks the HIP kernel: ``False`` the single pass (one block walks all keys of its rows), ``True``
    the key split of csrc/kernels/attention_extend_split.hip (fixed key chunks, fp32 partials, an ordered
    combine), ``None`` by plan: ``attn_extend_plan`` chooses from (B, T, Hq, Hkv, D, cap, CU count) alone, never
    from device data -- the split for a short append over a long cache, where the single pass leaves most CUs
    idle. For a fixed setting a sequence's result is a pure function of its own q, K, V, ``kv_len[b]`` and T
    (not of cap, the batch or the other lengths) with the same bits run to run; the two settings differ only
    in fp32 summation order. The torch-math path ignores it.

    With ``k_scale`` / ``v_scale`` the caches are fp8 (uint8, the new rows quantized by :func:`rope_append`) and
    the keys are their dequantized rows, a query's own row and the other new rows included:
    csrc/kernels/attention_extend_fp8.hip, which converts the bytes once while staging them and is the 16-bit
    kernel from there on. Same ``split``, same plan, same contract. uint8 scales mark an fp4 cache (caches
    [B, cap, Hkv, D / 2], scales [B, cap, Hkv, D / 32]): csrc/kernels/attention_extend_fp4.hip, the same with the
    nibbles converted at staging.

    With ``block_table`` / ``cap`` the caches are the pools of a :class:`PagedKVCache`: ``attn_extend_paged``, both
    arms, the same plan (it does not depend on paging), bit-equal to the dense kernel at the same ``split`` on the
    gathered cache."""
    scale = scale if scale is not None else 1.0 / math.sqrt(q.shape[-1])
    fp8, fp4 = _scale_kind(k_scale)
    if block_table is not None:
        if _decode_hip(q, q.shape[-1]):
            sp = -1 if split is None else int(bool(split))
            o, lse = _ext.require_for(q).attn_extend_paged(q, k_cache, v_cache, block_table, kv_len, cap, scale, sp)
            return o, lse
        o, lse = ref.attention_extend_paged_ref(q, k_cache, v_cache, block_table, kv_len, cap, scale)
        return o.to(q.dtype), lse
    if _decode_hip(q, q.shape[-1]):
        C, sp = _ext.require_for(q), -1 if split is None else int(bool(split))
        if fp4:
            o, lse = C.attn_extend_fp4(q, k_cache, v_cache, k_scale, v_scale, kv_len, scale, sp)
        elif fp8:
            o, lse = C.attn_extend_fp8(q, k_cache, v_cache, k_scale, v_scale, kv_len, scale, sp)
        else:
            o, lse = C.attn_extend(q, k_cache, v_cache, kv_len, scale, sp)
        return o, lse
    if fp4:
        o, lse = ref.attention_extend_fp4_ref(q, k_cache, v_cache, k_scale, v_scale, kv_len, scale)
    elif fp8:
        o, lse = ref.attention_extend_fp8_ref(q, k_cache, v_cache, k_scale, v_scale, kv_len, scale)
    else:
        o, lse = ref.attention_extend_ref(q, k_cache, v_cache, kv_len, scale)
    return o.to(q.dtype), lse


def _store_prompt_kv(k, v, kc, vc, ks, vs, block_table=None, cap=None) -> None:
    """The k / v views [B, S, Hkv, D] of the fused QKV activation into cache rows 0 .. S - 1 (with ``block_table``:
    logical rows of a paged cache; prompt padding beyond a sequence's mapped pages goes nowhere)."""
    S = k.shape[1]
    if block_table is not None:
        if _decode_hip(k, k.shape[-1]):
            _ext.require_for(k).kv_store_paged_(k, v, kc, vc, block_table, cap)
        else:
            ref.kv_store_paged_ref(k, v, kc, vc, block_table, cap)
    elif ks is None:
        kc[:, :S].copy_(k)  # strided copies
        vc[:, :S].copy_(v)
    elif _decode_hip(k, k.shape[-1]):
        C = _ext.require_for(k)
        (C.kv_quantize_fp4_ if ks.dtype == torch.uint8 else C.kv_quantize_)(k, v, kc, vc, ks, vs)
    else:
        quantize = ref.kv_quantize_fp4_ref if ks.dtype == torch.uint8 else ref.kv_quantize_ref
        kc[:, :S], ks[:, :S] = quantize(k)
        vc[:, :S], vs[:, :S] = quantize(v)


# ---------------------------------------------------------------------------------------
def _qkv_params(at):
    return [at.wq.weight, at.wk.weight, at.wv.weight]


def _prefill_attention(model, layer, n1, B: int, S: int, kc, vc, ks=None, vs=None, **paged):
    """The forward of ops/fused.py ``_AttentionBlock`` (same kernels, same rounding points), which also
    leaves the rotated k and the plain v of positions 0 .. S - 1 in the cache (quantized when the cache is
    fp8; the attention itself runs on the unquantized k and v)."""
    a = model.model_args
    Hq, Hkv, D = a.n_heads, a.kv_heads, a.head_dim
    at = layer.attention
    w_qkv, w_o = model._weight(_qkv_params(at)), model._weight([at.wo.weight])
    tab = model.rope_tab
    T = B * S
    x2 = n1.reshape(T, n1.shape[-1])
    nq, nk = Hq * D, Hkv * D
    if F._nt_ok(x2, w_qkv, "qkv") and D % 8 == 0 and tab.is_contiguous():
        qkv = torch.empty(T, w_qkv.size(0), dtype=x2.dtype, device=x2.device)
        _ext.require_for(x2).gemm_nt_(x2, w_qkv, qkv, 3, None, tab, S, D, nq + nk)
    else:
        qkv = torch.mm(x2, w_qkv.t())
        if _ext.hip(qkv) and D % 8 == 0:
            _ext.require_for(qkv).rope_(qkv, nq + nk, tab, D, S, 0, False, None)
        else:
            ref.rope_inplace_2d(qkv, nq + nk, tab, D, S)
    q = qkv[:, :nq].view(B, S, Hq, D)
    k = qkv[:, nq:nq + nk].view(B, S, Hkv, D)
    v = qkv[:, nq + nk:].view(B, S, Hkv, D)
    _store_prompt_kv(k, v, kc, vc, ks, vs, **paged)
    o, _ = F._attn_fwd(q, k, v, 1.0 / math.sqrt(D), True)
    return F._mm_nt(o.view(T, nq), w_o, "o").view(B, S, -1)


def _mlp(model, layer, n2):
    ff = layer.feed_forward
    up = [ff.w1.weight, ff.w3.weight]
    return F.swiglu_mlp(n2, model._weight(up), model._weight([ff.w2.weight]), model._slot(up),
                        model._slot([ff.w2.weight]), up + [ff.w2.weight])


def _head(model, h, pending):
    """Final norm (with the last block's pending residual add) and the output GEMM on rows [B, dim]."""
    if pending is None:
        nf = model._norm(model.norm, h, None)
    else:
        _, nf = model._norm(model.norm, h, pending)
    return torch.nn.functional.linear(nf, model.output.weight)


def _check_cache(model, cache, B: int):
    a = model.model_args
    if isinstance(cache, PagedKVCache) and tuple(cache.block_table.shape) != (cache.batch, cache.pages_per_seq):
        raise ValueError("PagedKVCache: the block table must be [batch, ceil(capacity / page_size)]")
    fp4 = getattr(cache, "fp4", False)
    row = a.head_dim // 2 if fp4 else a.head_dim
    if cache.batch != B or len(cache.k) != a.n_layers or tuple(cache.k[0].shape[2:]) != (a.kv_heads, row):
        raise ValueError("KVCache does not match the model / batch")
    w = model.tok_embeddings.weight
    kind = getattr(cache, "fp8", False) or fp4
    dtype = cache.dtype if kind else cache.k[0].dtype
    if dtype != w.dtype or cache.k[0].device != w.device:
        raise ValueError(f"KVCache is {dtype} on {cache.k[0].device}, the model {w.dtype} on {w.device}")
    if fp4 and (cache.k[0].dtype != torch.uint8 or cache.k_scale[0] is None or cache.k_scale[0].dtype != torch.uint8 or
                tuple(cache.k_scale[0].shape) != tuple(cache.k[0].shape[:-1]) + (a.head_dim // 32,)):
        raise ValueError("KVCache: an fp4 cache holds uint8 k / v [B, capacity, Hkv, D / 2] and uint8 scales "
                         "[B, capacity, Hkv, D / 32]")
    if kind and not fp4 and (cache.k[0].dtype != torch.uint8 or cache.k_scale[0] is None or
                 tuple(cache.k_scale[0].shape) != tuple(cache.k[0].shape[:-1])):
        raise ValueError("KVCache: an fp8 cache holds uint8 k / v and fp32 scales [B, capacity, Hkv]")


def _refuse_fp8(cache: KVCache, what: str, fp8_extend: bool = False, fp4_extend: bool = False) -> None:
    if getattr(cache, "fp4", False) and not fp4_extend:
        raise ValueError(f"{what} does not serve an fp4 KV cache, with or without fp8_extend: the prompt's attention "
                         f"is defined as unquantized (prefill). Opt in with fp4_extend=True (generate.py --fp4-extend): "
                         f"the new tokens are quantized into the cache first and every query attends to dequantized "
                         f"rows, as in decode_step")
    if getattr(cache, "fp8", False) and not fp8_extend:
        raise ValueError(f"{what} does not serve an fp8 KV cache: the prompt's attention is defined as unquantized "
                         f"(prefill), and new tokens attending to their own dequantized keys would change that. "
                         f"Opt in with fp8_extend=True (generate.py --fp8-extend): the new tokens are quantized "
                         f"into the cache first and every query attends to dequantized rows, as in decode_step")


def _extend_layers(model, tokens: torch.Tensor, cache: KVCache):
    """tokens [B, T] through every layer as an append at ``cache.kv_len`` (left unchanged): per layer the QKV
    GEMM on [B * T, dim], the T-token ``rope_append``, ``attn_extend``, W_o and the MLP, with the rounding
    points of ``decode_step``. An fp8 cache (the callers have checked the opt-in) passes its layer's scales to
    both ops. Returns (h, pending) [B, T, dim] for :func:`_head`."""
    B, T = tokens.shape
    a = model.model_args
    Hq, Hkv, D = a.n_heads, a.kv_heads, a.head_dim
    nq = Hq * D
    scale = 1.0 / math.sqrt(D)
    emb = model.tok_embeddings.weight
    h = F.embedding(tokens.contiguous(), emb, model._slot([emb]))
    pending = None
    paged = _paged_kw(cache)
    for i, layer in enumerate(model.layers.values()):
        if pending is None:
            x, n1 = h, model._norm(layer.attention_norm, h, None)
        else:
            x, n1 = model._norm(layer.attention_norm, h, pending)
        at = layer.attention
        qkv = torch.mm(n1.reshape(B * T, n1.shape[-1]), model._weight(_qkv_params(at)).t())
        ks, vs = cache.k_scale[i], cache.v_scale[i]  # None for a cache in the model's dtype
        rope_append(qkv, model.rope_tab, cache.kv_len, cache.k[i], cache.v[i], ks, vs, **paged)
        o, _ = attention_extend(qkv[:, :nq].view(B, T, Hq, D), cache.k[i], cache.v[i], cache.kv_len, scale,
                                k_scale=ks, v_scale=vs, **paged)
        att = F._mm_nt(o.view(B * T, nq), model._weight([at.wo.weight]), "o").view(B, T, -1)
        h, n2 = model._norm(layer.ffn_norm, x, att)
        pending = _mlp(model, layer, n2)
    return h, pending


@torch.no_grad()
def extend(model, tokens: torch.Tensor, n_new: torch.Tensor, cache: KVCache, return_all: bool = False,
           fp8_extend: bool = False, fp4_extend: bool = False) -> torch.Tensor:
    """Append ``n_new[b]`` tokens (``tokens`` [B, T] right-padded, 1 <= n_new[b] <= T, values outside are
    clamped) to every sequence at its own ``kv_len[b]`` -> logits [B, V] of row n_new[b] - 1, the next
    position's; ``kv_len += n_new`` (clamped at the capacity). A follow-up turn, a continuation after a
    shared prefix, one piece of a chunked prefill, the pass a speculative verifier needs.

    All T rows are computed: the pad rows' k / v land beyond the new ``kv_len`` and are overwritten by
    whatever is appended next, as prompt padding is in :func:`prefill`. A token whose position is at or
    beyond the capacity stores nothing and attends to the whole cache (T = 1 overwrites the last row, as
    ``decode_step`` does). ``n_new`` and ``kv_len`` stay on the device: no host synchronisation.
    ``return_all=True`` returns the logits of every row, [B, T, V], instead (scoring; pad rows included).

    An fp8 cache is refused with ``ValueError`` unless ``fp8_extend=True``. With it an append does, per layer,
    what ``decode_step`` does for one token: the T new tokens' rotated k and plain v are quantized into the
    cache first, then query t attends to the dequantized cache rows 0 .. min(kv_len[b] + t, cap - 1), its own
    row and the other new rows included. So ``extend`` with T = 1 is ``decode_step``, and with T tokens it
    equals T ``decode_step`` calls in exact arithmetic. The flag is ignored for a cache in the model's dtype.
    An fp4 cache is refused with ``ValueError`` whatever ``fp8_extend`` says; ``fp4_extend=True`` serves it by the
    same rule (the T-token ``rope_append_fp4``, then ``attn_extend_fp4`` over the dequantized rows), and is ignored
    for any other cache.

    On a forked :class:`PagedKVCache` ``extend`` and the chunked prefill keep using ``attn_extend_paged`` per
    sequence: only ``decode_step`` reads a group's shared pages once."""
    if tokens.dim() != 2 or tokens.shape[1] < 1:
        raise ValueError(f"extend: tokens must be [B, T] with T >= 1, got {tuple(tokens.shape)}")
    B, T = tokens.shape
    _check_cache(model, cache, B)
    _refuse_fp8(cache, "extend", fp8_extend, fp4_extend)
    n_new = n_new.to(device=tokens.device, dtype=torch.long).clamp(1, T)
    h, pending = _extend_layers(model, tokens, cache)
    cache.kv_len.copy_((cache.kv_len + n_new).clamp(max=cache.capacity))
    if return_all:
        return _head(model, h, pending)
    bi = torch.arange(B, device=tokens.device)
    rows = n_new - 1
    return _head(model, h[bi, rows].contiguous(), None if pending is None else pending[bi, rows].contiguous())


def _prefill_chunked(model, tokens: torch.Tensor, lens: torch.Tensor, cache: KVCache, chunk: int) -> torch.Tensor:
    """:func:`prefill` in pieces of ``chunk`` columns, each an append onto the cache so far at the uniform base
    c0 (``kv_len`` is set to it before the piece). The rows lens[b] - 1 are picked out of the piece they
    fall in with a select on the device; the head runs once, on those B rows."""
    B, S = tokens.shape
    rows = (lens - 1).clamp(0, S - 1)
    bi = torch.arange(B, device=tokens.device)
    h_sel = p_sel = None
    for c0 in range(0, S, chunk):
        piece = tokens[:, c0:c0 + chunk]
        cache.kv_len.fill_(c0)
        h, pending = _extend_layers(model, piece, cache)
        local = (rows - c0).clamp(0, piece.shape[1] - 1)
        here = ((rows >= c0) & (rows < c0 + piece.shape[1])).unsqueeze(-1)
        hr = h[bi, local]
        h_sel = hr if h_sel is None else torch.where(here, hr, h_sel)
        if pending is not None:
            pr = pending[bi, local]
            p_sel = pr if p_sel is None else torch.where(here, pr, p_sel)
    cache.kv_len.copy_(lens.clamp(0, cache.capacity))
    return _head(model, h_sel.contiguous(), None if p_sel is None else p_sel.contiguous())


@torch.no_grad()
def prefill(model, tokens: torch.Tensor, lens: torch.Tensor, cache: KVCache, chunk: int = 0,
            fp8_extend: bool = False, fp4_extend: bool = False) -> torch.Tensor:
    """tokens [B, S] (ragged prompts right-padded), lens [B] in 1 .. S -> logits [B, V] of row
    lens[b] - 1 of each sequence. Fills the cache rows 0 .. S - 1 and sets kv_len = lens. Causal
    attention makes every position below lens[b] independent of the padding; no [B, S, V] logits exist.

    With an fp8 cache the attention over the prompt still runs on the unquantized k / v; only what is
    stored is quantized. The logits returned here, the first generated token's, are therefore bit-equal to
    those of the ``"model"`` cache, and ``prefill(p)`` + ``decode_step(t)`` and ``prefill(p + t)`` see
    different keys for the prompt: dequantized ones in the first, the 16-bit ones in the second.

    ``chunk > 0`` feeds the prompt in pieces of ``chunk`` columns, each an append onto the cache so far
    (the layer body of :func:`extend`): peak activation memory scales with B * chunk, not B * S, and the
    result is the one-shot prefill's up to summation order. It refuses an fp8 cache (``ValueError``): a
    piece would attend to dequantized keys. ``fp8_extend=True`` opts into exactly that (see :func:`extend`):
    every piece attends to dequantized rows, so the result differs from the one-shot prefill by quantization
    error, not only by summation order. ``chunk = 0`` is the one-shot path, with or without the flag. An fp4
    cache is the same story under its own flag: ``chunk > 0`` refuses it whatever ``fp8_extend`` says and serves it
    with ``fp4_extend=True``."""
    B, S = tokens.shape
    _check_cache(model, cache, B)
    if S > cache.capacity:
        raise ValueError(f"prompt length {S} exceeds the cache capacity {cache.capacity}")
    lens = lens.to(device=tokens.device, dtype=torch.long)
    if chunk < 0:
        raise ValueError(f"prefill: chunk must be >= 0, got {chunk}")
    if chunk > 0:
        _refuse_fp8(cache, "prefill(chunk > 0)", fp8_extend, fp4_extend)
        return _prefill_chunked(model, tokens, lens, cache, int(chunk))
    emb = model.tok_embeddings.weight
    h = F.embedding(tokens, emb, model._slot([emb]))
    pending = None
    paged = _paged_kw(cache)
    for i, layer in enumerate(model.layers.values()):
        if pending is None:
            x, n1 = h, model._norm(layer.attention_norm, h, None)
        else:
            x, n1 = model._norm(layer.attention_norm, h, pending)
        att = _prefill_attention(model, layer, n1, B, S, cache.k[i], cache.v[i], cache.k_scale[i], cache.v_scale[i],
                                 **paged)
        h, n2 = model._norm(layer.ffn_norm, x, att)
        pending = _mlp(model, layer, n2)
    cache.kv_len.copy_(lens.clamp(0, cache.capacity))
    rows = (lens - 1).clamp(0, S - 1)
    bi = torch.arange(B, device=tokens.device)
    return _head(model, h[bi, rows].contiguous(), None if pending is None else pending[bi, rows].contiguous())


@torch.no_grad()
def decode_step(model, tokens: torch.Tensor, cache: KVCache) -> torch.Tensor:
    """One token per sequence (tokens [B], the token at position kv_len[b]) -> logits [B, V] for the
    next position; kv_len grows by one (clamped at the capacity). No host synchronisation. On a forked
    :class:`PagedKVCache` the attention reads a group's shared pages once (``attn_decode_shared_paged``)."""
    B = tokens.shape[0]
    _check_cache(model, cache, B)
    a = model.model_args
    Hq, Hkv, D = a.n_heads, a.kv_heads, a.head_dim
    nq = Hq * D
    scale = 1.0 / math.sqrt(D)
    # once per step, not per layer: the lengths the attention sees, the new token included
    att_len = (cache.kv_len + 1).clamp_(max=cache.capacity)
    emb = model.tok_embeddings.weight
    h = F.embedding(tokens.reshape(B, 1), emb, model._slot([emb])).view(B, -1)
    pending = None
    paged, group = _paged_kw(cache), _group_kw(cache)
    for i, layer in enumerate(model.layers.values()):
        if pending is None:
            x, n1 = h, model._norm(layer.attention_norm, h, None)
        else:
            x, n1 = model._norm(layer.attention_norm, h, pending)
        at = layer.attention
        qkv = torch.mm(n1, model._weight(_qkv_params(at)).t())
        ks, vs = cache.k_scale[i], cache.v_scale[i]  # None: a cache in the model's dtype
        rope_append(qkv, model.rope_tab, cache.kv_len, cache.k[i], cache.v[i], ks, vs, **paged)
        o, _ = attention_decode(qkv[:, :nq].view(B, Hq, D), cache.k[i], cache.v[i], att_len, scale, ks, vs, **paged,
                                **group)
        att = F._mm_nt(o.view(B, nq), model._weight([at.wo.weight]), "o")
        h, n2 = model._norm(layer.ffn_norm, x, att)
        pending = _mlp(model, layer, n2)
    cache.kv_len.copy_(att_len)
    return _head(model, h, pending)


# ---------------------------------------------------------------------------------------
def greedy_token(logits: torch.Tensor) -> torch.Tensor:
    """argmax over the last dim; ties go to the lowest token id."""
    V = logits.shape[-1]
    top = logits.max(dim=-1, keepdim=True).values
    ids = torch.arange(V, device=logits.device).expand_as(logits)
    return torch.where(logits == top, ids, V).min(dim=-1).values.clamp_(max=V - 1)


def filter_logits(logits: torch.Tensor, temperature: float, top_k: int = 0, top_p: float = 1.0) -> torch.Tensor:
    """fp32 logits / temperature with everything outside the top-k set and the top-p nucleus at -inf. The
    nucleus is the shortest prefix of the tokens sorted by probability whose mass reaches top_p."""
    x = logits.float() / temperature
    V = x.shape[-1]
    if 0 < top_k < V:
        kth = torch.topk(x, top_k, dim=-1).values[..., -1:]
        x = x.masked_fill(x < kth, float("-inf"))
    if top_p < 1.0:
        sx, si = torch.sort(x, dim=-1, descending=True, stable=True)
        p = torch.softmax(sx, dim=-1)
        before = torch.cumsum(p, dim=-1) - p  # mass of the tokens ranked above
        drop = before >= top_p
        drop[..., 0] = False  # the most likely token always stays
        x = x.masked_fill(torch.zeros_like(drop).scatter(-1, si, drop), float("-inf"))
    return x


def sample_token(logits: torch.Tensor, temperature: float = 0.0, top_k: int = 0, top_p: float = 1.0,
                 generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """Next token ids [B] from logits [B, V]: greedy at temperature 0, else a draw from the filtered
    softmax of the fp32 logits with ``generator``."""
    if temperature == 0.0:
        return greedy_token(logits)
    probs = torch.softmax(filter_logits(logits, temperature, top_k, top_p), dim=-1)
    return torch.multinomial(probs, 1, generator=generator).squeeze(-1)


def _model_device_dtype(model):
    w = model.tok_embeddings.weight
    return w.device, w.dtype


def _seed64(seed: int) -> int:
    """Any Python int as the signed 64-bit value the binding takes (the kernel reads it as unsigned)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return seed - (1 << 64) if seed >= (1 << 63) else seed


def sample_philox(logits: torch.Tensor, pos: torch.Tensor, temperature: float = 0.0, top_k: int = 0,
                  top_p: float = 1.0, seed: int = 0) -> torch.Tensor:
    """Next token ids [B] from logits [B, V] by the stateless rule (``ops/reference.py::sample_philox_ref``
    documents it): row b draws with the Philox uniform of (seed, b, pos[b]), ``pos[b]`` being the absolute
    position the token will occupy. bf16 / fp16 logits on the GPU run the HIP kernel, everything else the
    torch rule."""
    if temperature < 0 or not 0.0 < top_p <= 1.0 or top_k < 0:
        raise ValueError("sample_philox: need temperature >= 0, 0 < top_p <= 1, top_k >= 0")
    if not _ext.hip16(logits):
        return ref.sample_philox_ref(logits, pos, temperature, top_k, top_p, seed)
    tok = torch.empty(logits.shape[0], dtype=torch.long, device=logits.device)
    pos = pos.to(device=logits.device, dtype=torch.int32).contiguous()
    _ext.require_for(logits).sample_(logits, tok, temperature, top_k, top_p, _seed64(seed), pos=pos)
    return tok


class DeviceSampler:
    """The sampling kernel with the generation state of one ``generate`` call on the device: ``out`` int64
    [B, max_new] (-1 where nothing was written), ``count`` int32 [B], ``done`` uint8 [B] and ``tok`` int64
    [B], the next decode step's input (0 for finished rows). ``room`` [B] is the number of cache rows a
    sequence has left after its prompt: the token that finds the cache full is emitted and finishes the
    row. One :meth:`sample` is one launch and reads nothing from the host; draws are indexed by
    ``prompt_len + count``. bf16 / fp16 logits on the GPU only."""

    def __init__(self, prompt_len: torch.Tensor, room: torch.Tensor, max_new_tokens: int, temperature: float = 0.0,
                 top_k: int = 0, top_p: float = 1.0, seed: int = 0, eos_id: Optional[int] = None):
        if temperature < 0 or not 0.0 < top_p <= 1.0 or top_k < 0 or max_new_tokens < 1:
            raise ValueError("DeviceSampler: need temperature >= 0, 0 < top_p <= 1, top_k >= 0, max_new_tokens >= 1")
        dev = prompt_len.device
        B = prompt_len.numel()
        self.C = _ext.require_for(prompt_len)
        self.args = (float(temperature), int(top_k), float(top_p), _seed64(seed))
        self.eos_id = -1 if eos_id is None else int(eos_id)
        self.prompt_len = prompt_len.to(torch.int32).contiguous()
        self.room = room.to(device=dev, dtype=torch.int32).contiguous()
        self.out = torch.full((B, max_new_tokens), -1, dtype=torch.long, device=dev)
        self.count = torch.zeros(B, dtype=torch.int32, device=dev)
        self.done = torch.zeros(B, dtype=torch.uint8, device=dev)
        self.tok = torch.zeros(B, dtype=torch.long, device=dev)
        self.ws = (torch.empty(self.C.sample_ws_bytes(B) // 4, dtype=torch.int32, device=dev)
                   if temperature > 0 else None)

    def sample(self, logits: torch.Tensor) -> torch.Tensor:
        self.C.sample_(logits, self.tok, *self.args, ws=self.ws, done=self.done, count=self.count, room=self.room,
                       out=self.out, eos_id=self.eos_id, prompt_len=self.prompt_len)
        return self.tok

    def all_done(self) -> bool:
        """Reads the finished mask back: a host synchronisation."""
        return bool(self.done.all().item())


class DecodeGraph:
    """One generated token per :meth:`step`: sample from the static ``logits`` buffer, ``decode_step`` the
    token, copy the new logits into the buffer. The first ``WARMUP`` steps run eagerly (library warm-up and
    GEMM tuning; their tokens are real), the next one captures the body into a hipGraph on one stream
    (a linear graph: the body forks no stream) and every step from there on is one replay. Temperature,
    top-k, top-p and the seed are constants of the capture; every per-token quantity (``kv_len``, the
    position of the draw, the finished mask) is read from device memory, so eager steps and replays give
    the same bits."""

    WARMUP = 2

    def __init__(self, model, cache: KVCache, logits: torch.Tensor, sampler: DeviceSampler):
        if not (_ext.hip16(logits) and model.model_args.head_dim in (64, 128)):
            raise ValueError("DecodeGraph needs a bf16 / fp16 GPU model on the HIP decode path (head_dim 64 or 128)")
        self.model, self.cache, self.sampler = model, cache, sampler
        self.logits = logits.detach().clone().contiguous()
        self.graph = None
        self.steps = 0

    @property
    def captured(self) -> bool:
        return self.graph is not None

    def _body(self):
        tok = self.sampler.sample(self.logits)
        self.logits.copy_(decode_step(self.model, tok, self.cache))

    def step(self) -> None:
        if self.steps < self.WARMUP:
            self._body()
        else:
            if self.graph is None:
                torch.cuda.synchronize()
                torch.cuda.empty_cache()  # eager-step blocks are not reusable by the graph's private pool
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):  # records without executing: the replay below runs this step
                    self._body()
                self.graph = g
            self.graph.replay()
        self.steps += 1


def _graph_refusal(model, device, dtype, sampler: str, temperature: float, use_cache: bool) -> Optional[str]:
    if sampler != "philox" and temperature != 0.0:
        return ("sampler='torch' draws with a torch.Generator, whose state lives outside a graph: use "
                "sampler='philox' or temperature 0")
    if not use_cache:
        return "the captured step is the KV-cache decode step: use_cache=False cannot be captured"
    if device.type != "cuda" or dtype not in (torch.bfloat16, torch.float16):
        return f"the captured step runs the HIP kernels: a bf16 / fp16 model on the GPU, not {dtype} on {device.type}"
    if model.model_args.head_dim not in (64, 128):
        return f"the HIP decode kernels take head_dim 64 or 128, not {model.model_args.head_dim}"
    return None


@torch.no_grad()
def generate(model, prompts: Sequence[Sequence[int]], max_new_tokens: int, temperature: float = 0.0, top_k: int = 0,
             top_p: float = 1.0, seed: int = 0, eos_id: Optional[int] = None, use_cache: bool = True,
             stats: Optional[Dict] = None, sampler: str = "torch", graph: bool = False,
             kv_cache_dtype: str = "model", prefill_chunk: int = 0, fp8_extend: bool = False,
             kv_page_size: int = 0, n_samples: int = 1, fp4_extend: bool = False) -> Tuple[List[List[int]], List[str]]:
    """Generate up to ``max_new_tokens`` tokens after each prompt (lists of token ids, ragged).

    Returns (generated ids per prompt, finish reason per prompt): ``eos`` (the last id is ``eos_id``),
    ``max_new_tokens``, or ``length`` when the sequence filled the cache (the model's ``seq_len``).
    ``temperature == 0`` is greedy (ties to the lowest id); otherwise fp32 logits are sampled with a
    ``torch.Generator`` on the model's device seeded by ``seed``: same seed, same device, same tokens.
    The finished mask lives on the device and is read back at most once per 16 generated tokens.
    ``use_cache=False`` is the naive path (a full ``model(tokens)`` per new token): a debugging aid and
    a second opinion. ``stats`` (a dict, optional) receives ``prefill_ms`` and ``decode_ms_per_token``
    from device events on a GPU model (wall clock on the CPU).

    ``sampler="philox"`` draws by the stateless rule of :func:`sample_philox` instead: the token at
    absolute position n of row b is a function of (seed, b, n) and the logits alone, on any device and on
    both the cache and the naive path. On a bf16 / fp16 GPU model with the cache, sampling and the
    bookkeeping are one kernel launch per token (:class:`DeviceSampler`). ``graph=True`` also replays
    sample -> ``decode_step`` as a hipGraph (:class:`DecodeGraph`); it needs ``sampler="philox"`` or
    temperature 0 and a bf16 / fp16 GPU model on the HIP decode path, and raises ``ValueError`` with the
    reason otherwise.

    ``kv_cache_dtype="fp8"`` keeps the cache as e4m3fn bytes with one power-of-two scale per (token, kv
    head) (:class:`KVCache`): about half the cache memory and half the bytes a decode step reads. The
    prompt's attention runs unquantized (:func:`prefill`), so the first generated token is the one the
    ``"model"`` cache gives; later tokens attend to dequantized keys and values. It needs the cache:
    ``use_cache=False`` raises ``ValueError``.

    ``kv_cache_dtype="fp4"`` keeps it as OCP MXFP4 (e2m1 nibbles, one power-of-two scale per 32 columns): about
    half of the fp8 cache again, under the same rules (the first generated token is the ``"model"`` cache's). It
    does not combine with ``kv_page_size``, and with ``prefill_chunk`` only under ``fp4_extend=True``.

    ``prefill_chunk=N`` (N > 0) feeds the prompt through :func:`prefill` in pieces of N columns, bounding the
    prefill's activation memory by B * N rows; the tokens are those of the one-shot prefill up to summation
    order. It needs the cache and refuses ``kv_cache_dtype="fp8"`` unless ``fp8_extend=True``: then every piece
    attends to dequantized cache rows (:func:`extend`), and the tokens differ from the one-shot prefill's by
    quantization error too. The flag does nothing for a ``"model"`` cache. ``fp4_extend=True`` is the same opt-in
    for ``kv_cache_dtype="fp4"`` (csrc/kernels/attention_extend_fp4.hip). ``stats["prefill_chunks"]`` is the
    number of pieces (0: the one-shot prefill).

    ``kv_page_size=N`` (64, 128 or 256; 0, the default, is the dense cache exactly as before) keeps the cache in
    pages of N tokens (:class:`PagedKVCache`, csrc/kernels/attention_paged.hip) with the same logical capacity:
    sequence b gets ``ceil(min(cap, len_b + max_new_tokens) / N)`` pages, reserved before the prefill, instead of
    the longest sequence's rows, so a ragged batch pays for what it can use. The tokens are the dense cache's
    (the paged kernels return its bits) and the table is static while decoding, so ``graph=True`` works. It needs
    ``use_cache=True`` and ``kv_cache_dtype="model"``. ``stats["kv_cache_bytes"]`` is the cache's allocation, for
    both layouts (0 without a cache).

    ``n_samples=N`` (N > 1) draws N samples per prompt and returns them prompt-major: index ``p * N + i`` is sample
    i of prompt p. The B prompts are prefilled once; :meth:`PagedKVCache.fork` then gives every prompt N rows
    that name its full pages (the pool holds them once, plus each sample's own pages), every sample's first
    token is drawn from the prompt's logits, and decoding runs on B * N rows whose attention reads a prompt's
    shared pages once per step (csrc/kernels/attention_decode_shared.hip). ``sampler="philox"`` keys its draws on
    the row, so the samples of a prompt differ; greedy samples are identical. It needs ``kv_page_size != 0`` and
    ``use_cache=True``. ``stats["n_samples"]`` records N."""
    if n_samples < 1 or (n_samples > 1 and not (kv_page_size and use_cache)):
        raise ValueError("generate: n_samples must be >= 1, and n_samples > 1 needs the paged KV cache "
                         "(kv_page_size != 0, use_cache=True): the samples of a prompt share its pages")
    if temperature < 0 or not 0.0 < top_p <= 1.0 or top_k < 0 or max_new_tokens < 1:
        raise ValueError("generate: need temperature >= 0, 0 < top_p <= 1, top_k >= 0, max_new_tokens >= 1")
    if sampler not in ("torch", "philox"):
        raise ValueError(f"generate: sampler must be 'torch' or 'philox', got {sampler!r}")
    if kv_cache_dtype not in KV_DTYPES:
        raise ValueError(f"generate: kv_cache_dtype must be one of {KV_DTYPES}, got {kv_cache_dtype!r}")
    if kv_cache_dtype != "model" and not use_cache:
        raise ValueError(f"generate: kv_cache_dtype={kv_cache_dtype!r} needs the KV cache (use_cache=True)")
    if kv_page_size != 0 and kv_page_size not in PAGE_SIZES:
        raise ValueError(f"generate: kv_page_size must be 0 (the dense cache) or one of {PAGE_SIZES}, got {kv_page_size}")
    if kv_page_size and use_cache and kv_cache_dtype == "fp4":
        raise ValueError("generate: kv_page_size needs kv_cache_dtype='model': a paged fp4 cache is a follow-up")
    if kv_page_size and (not use_cache or kv_cache_dtype != "model"):
        raise ValueError("generate: kv_page_size needs the KV cache (use_cache=True) in the model's dtype "
                         "(kv_cache_dtype='model'): a paged fp8 cache is a follow-up")
    if prefill_chunk < 0 or (prefill_chunk > 0 and not use_cache):
        raise ValueError("generate: prefill_chunk must be >= 0 and needs the KV cache (use_cache=True)")
    device, dtype = _model_device_dtype(model)
    if graph:
        why = _graph_refusal(model, device, dtype, sampler, temperature, use_cache)
        if why is not None:
            raise ValueError("generate: graph=True refused: " + why)
    args = model.model_args
    B = len(prompts)
    lens_host = [len(p) for p in prompts]
    if B == 0 or min(lens_host) < 1:
        raise ValueError("generate: every prompt needs at least one token")
    S = max(lens_host)
    if S > args.seq_len:
        raise ValueError(f"generate: prompt length {S} exceeds the model's seq_len {args.seq_len}")
    cap = min(args.seq_len, S + max_new_tokens)
    buf = torch.zeros(B, cap, dtype=torch.long)
    for b, p in enumerate(prompts):
        buf[b, :len(p)] = torch.as_tensor(list(p), dtype=torch.long)
    buf = buf.to(device)
    lens = torch.tensor(lens_host, dtype=torch.long, device=device)
    room = cap - lens  # [B]: tokens a sequence can still append
    gen = None
    if temperature > 0 and sampler == "torch":
        gen = torch.Generator(device=device)
        gen.manual_seed(int(seed))
    # sampling and bookkeeping in one launch per token: the philox rule (or greedy, for a graph) on 16-bit GPU logits
    on_device = use_cache and _ext.hip16(model.tok_embeddings.weight) and (sampler == "philox" or graph)

    timer = _Timer(device)
    timer.mark()
    cache = None
    if use_cache and kv_page_size:
        need = [min(cap, n + max_new_tokens) for n in lens_host]  # tokens a sequence can ever hold
        pages = [-(-n // kv_page_size) for n in need]
        # a further sample names the prompt's full pages again and owns the rest
        own = [p - n // kv_page_size for p, n in zip(pages, lens_host)]
        cache = PagedKVCache(args, B, cap, dtype, device, kv_page_size, sum(pages) + (n_samples - 1) * sum(own))
        for b, n in enumerate(need):
            cache.reserve(b, n)
    elif use_cache:
        cache = KVCache(args, B, cap, dtype, device, kv_cache_dtype)
    if use_cache:
        logits = prefill(model, buf[:, :S], lens, cache, chunk=prefill_chunk, fp8_extend=fp8_extend,
                         fp4_extend=fp4_extend)
    else:
        bi = torch.arange(B, device=device)
        logits = model(buf[:, :S])[bi, lens - 1]
    if n_samples > 1:  # from here on B * n_samples rows, prompt-major: the samples of a prompt are one group
        cache = cache.fork(n_samples, lens_host)
        for b in range(B * n_samples):
            cache.reserve(b, need[b // n_samples])
        B *= n_samples
        logits, lens, room = (x.repeat_interleave(n_samples, 0) for x in (logits, lens, room))
    timer.mark()

    steps = 0
    if on_device:
        dsamp = DeviceSampler(lens, room, max_new_tokens, temperature, top_k, top_p, seed, eos_id)
        dgraph = DecodeGraph(model, cache, logits, dsamp) if graph else None
        for i in range(max_new_tokens):
            if i + 1 == max_new_tokens:
                dsamp.sample(dgraph.logits if graph else logits)  # the last token needs no decode step after it
                break
            if graph:
                dgraph.step()
            else:
                tok = dsamp.sample(logits)
                if (i + 1) % SYNC_EVERY == 0 and dsamp.all_done():
                    break
                logits = decode_step(model, tok, cache)
            steps += 1
            if graph and (i + 1) % SYNC_EVERY == 0 and dsamp.all_done():
                break
        out, count = dsamp.out, dsamp.count
    else:
        out = torch.full((B, max_new_tokens), -1, dtype=torch.long, device=device)
        count = torch.zeros(B, dtype=torch.long, device=device)
        done = torch.zeros(B, dtype=torch.bool, device=device)
        for i in range(max_new_tokens):
            if sampler == "philox":  # the token lands at absolute position lens + i (finished rows: unused)
                tok = sample_philox(logits, lens + i, temperature, top_k, top_p, seed)
            else:
                tok = sample_token(logits, temperature, top_k, top_p, gen)
            out[:, i] = torch.where(done, out[:, i], tok)
            count += (~done).long()
            if eos_id is not None:
                done = done | (tok == eos_id)
            done = done | (room <= i)  # token i was the last this sequence has a cache row for
            if i + 1 == max_new_tokens:
                break
            if (i + 1) % SYNC_EVERY == 0 and bool(done.all().item()):
                break
            tok = torch.where(done, torch.zeros_like(tok), tok)
            if use_cache:
                logits = decode_step(model, tok, cache)
            else:
                col = (lens + i).clamp(max=cap - 1)
                keep = buf.gather(1, col[:, None])[:, 0]
                buf.scatter_(1, col[:, None], torch.where(done, keep, tok)[:, None])
                L = min(S + i + 1, cap)
                logits = model(buf[:, :L])[bi, (lens + i + 1).clamp(max=L) - 1]
            steps += 1
    timer.mark()
    if stats is not None:
        t = timer.intervals_ms()
        stats["prefill_ms"] = t[0]
        stats["decode_ms_per_token"] = t[1] / steps if steps else 0.0
        stats["decode_steps"] = steps
        stats["prefill_chunks"] = -(-S // prefill_chunk) if prefill_chunk > 0 else 0
        stats["kv_cache_bytes"] = cache.nbytes() if cache is not None else 0
        stats["n_samples"] = n_samples
        stats["graph_replays"] = max(0, dgraph.steps - DecodeGraph.WARMUP) if graph else 0

    out_h, count_h = out.cpu(), count.cpu().tolist()
    tokens, reasons = [], []
    for b in range(B):
        ids = out_h[b, :count_h[b]].tolist()
        tokens.append(ids)
        if eos_id is not None and ids and ids[-1] == eos_id:
            reasons.append("eos")
        elif len(ids) == max_new_tokens:
            reasons.append("max_new_tokens")
        else:
            reasons.append("length")
    return tokens, reasons


class _Timer:
    """Marks on the current stream (device events on a GPU, the wall clock on the CPU)."""

    def __init__(self, device):
        self.cuda = device.type == "cuda"
        self.marks = []

    def mark(self):
        if self.cuda:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            self.marks.append(e)
        else:
            import time

            self.marks.append(time.perf_counter())

    def intervals_ms(self) -> List[float]:
        if self.cuda:
            self.marks[-1].synchronize()
            return [a.elapsed_time(b) for a, b in zip(self.marks, self.marks[1:])]
        return [(b - a) * 1e3 for a, b in zip(self.marks, self.marks[1:])]
