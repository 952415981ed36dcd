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
``prefill(chunk=N)`` feeds a prompt through it in pieces of N columns, so the prefill's activation memory
is bounded by the piece. fp8 caches are refused by both.

The HIP decode kernels take bf16 / fp16 at head_dim 64 / 128. CPU tensors, fp32 / fp64 models on the
GPU and other head dims run the torch math of :mod:`pyrecover_amd.ops.reference`
(``attention_decode_ref`` / ``attention_extend_ref`` / ``rope_append_ref``), noted once through
``_note_fallback`` like attention.

``KVCache(kv_dtype="fp8")`` (``generate(kv_cache_dtype="fp8")``) keeps k / v as OCP e4m3fn bytes with one
power-of-two scale per (token, kv head), about half the cache's memory and half the bytes a decode step
reads: csrc/kernels/attention_decode_fp8.hip (``kv_quantize``, ``rope_append_fp8``, ``attn_decode_fp8``), the
rule in ``ops/reference.py::kv_quantize_ref``. The prompt's attention stays unquantized; only what is stored
is quantized. Opt-in: without it nothing changes.

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


KV_DTYPES = ("model", "fp8")


class KVCache:
    """Per-layer k / v of shape [B, capacity, Hkv, D] (token-major, like every activation here) and the
    int32 device tensor ``kv_len`` [B] of tokens held per sequence.

    ``kv_dtype="model"`` (the default) stores k / v in ``dtype``. ``kv_dtype="fp8"`` stores every head row
    as D bytes of OCP e4m3fn (uint8 tensors ``k`` / ``v``) and one power-of-two fp32 scale (``k_scale`` /
    ``v_scale`` [B, capacity, Hkv]) by the rule of ``ops/reference.py::kv_quantize_ref``: (D + 4) / (2 D)
    of the 16-bit cache's bytes. ``dtype`` stays the model's dtype: the dtype of q and of the output."""

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
        self.fp8 = kv_dtype == "fp8"
        shape = (model_args.n_layers, batch, capacity, model_args.kv_heads, model_args.head_dim)
        self._k = torch.zeros(shape, dtype=torch.uint8 if self.fp8 else dtype, device=device)
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
        self.kv_len = torch.zeros(batch, dtype=torch.int32, device=device)

    def nbytes(self) -> int:
        n = 2 * self._k.numel() * self._k.element_size()
        return n + 2 * self._k_scale.numel() * 4 if self.fp8 else n


def _decode_hip(qkv: torch.Tensor, head_dim: int) -> bool:
    return F._note_fallback("decode attention", qkv, _ext.hip16(qkv) and head_dim in (64, 128))


def rope_append(qkv, tab, kv_len, k_cache, v_cache, k_scale=None, v_scale=None) -> None:
    """The new tokens' fused QKV rows [B * T, (Hq + 2 Hkv) D], T per sequence (B is the caches'): row
    b * T + t has q rotated in place at position kv_len[b] + t, rotated k and plain v into that cache row.
    Bit-equal to ``rope_`` on the same row at that position. T = 1 clamps the row to cap - 1; with T > 1 a
    position at or beyond the capacity stores nothing (its q takes table row cap - 1).
    With ``k_scale`` / ``v_scale`` the caches are fp8 (uint8): the same rows are quantized on the way in
    (T = 1 only)."""
    fp8 = k_scale is not None
    if fp8 and qkv.shape[0] != k_cache.shape[0]:
        raise ValueError("rope_append: an fp8 cache takes one token per sequence (extend does not serve fp8 caches)")
    if _decode_hip(qkv, k_cache.shape[-1]):
        C = _ext.require_for(qkv)
        if fp8:
            C.rope_append_fp8_(qkv, tab, kv_len, k_cache, v_cache, k_scale, v_scale)
        else:
            C.rope_append_(qkv, tab, kv_len, k_cache, v_cache)
    elif fp8:
        ref.rope_append_fp8_ref(qkv, tab, kv_len, k_cache, v_cache, k_scale, v_scale)
    else:
        ref.rope_append_ref(qkv, tab, kv_len, k_cache, v_cache)


def attention_decode(q, k_cache, v_cache, kv_len, scale: Optional[float] = None, k_scale=None,
                     v_scale=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """q [B, Hq, D] over the caches [B, cap, Hkv, D]: sequence b attends to keys 0 .. kv_len[b] - 1.
    Returns (o [B, Hq, D] in q's dtype, lse fp32 [B, Hq] -- the opmath dtype on the torch path).
    With ``k_scale`` / ``v_scale`` the caches are fp8 (uint8) and the keys are their dequantized rows."""
    scale = scale if scale is not None else 1.0 / math.sqrt(q.shape[-1])
    fp8 = k_scale is not None
    if _decode_hip(q, q.shape[-1]):
        C = _ext.require_for(q)
        if fp8:
            o, lse = C.attn_decode_fp8(q, k_cache, v_cache, k_scale, v_scale, kv_len, scale)
        else:
            o, lse = C.attn_decode(q, k_cache, v_cache, kv_len, scale)
        return o, lse
    if fp8:
        o, lse = ref.attention_decode_fp8_ref(q, k_cache, v_cache, k_scale, v_scale, kv_len, scale)
    else:
        o, lse = ref.attention_decode_ref(q, k_cache, v_cache, kv_len, scale)
    return o.to(q.dtype), lse


def attention_extend(q, k_cache, v_cache, kv_len, scale: Optional[float] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """q [B, T, Hq, D] over the caches [B, cap, Hkv, D], which hold the T new tokens' k / v already
    (:func:`rope_append` first); ``kv_len`` [B] counts the tokens held before the append. Query t of
    sequence b attends to keys 0 .. min(kv_len[b] + t, cap - 1). Returns (o [B, T, Hq, D] in q's dtype,
    lse fp32 [B, T, Hq] -- the opmath dtype on the torch path)."""
    scale = scale if scale is not None else 1.0 / math.sqrt(q.shape[-1])
    if _decode_hip(q, q.shape[-1]):
        o, lse = _ext.require_for(q).attn_extend(q, k_cache, v_cache, kv_len, scale)
        return o, lse
    o, lse = ref.attention_extend_ref(q, k_cache, v_cache, kv_len, scale)
    return o.to(q.dtype), lse


def _store_prompt_kv(k, v, kc, vc, ks, vs) -> None:
    """The k / v views [B, S, Hkv, D] of the fused QKV activation into cache rows 0 .. S - 1."""
    S = k.shape[1]
    if ks is None:
        kc[:, :S].copy_(k)  # strided copies
        vc[:, :S].copy_(v)
    elif _decode_hip(k, k.shape[-1]):
        _ext.require_for(k).kv_quantize_(k, v, kc, vc, ks, vs)
    else:
        kc[:, :S], ks[:, :S] = ref.kv_quantize_ref(k)
        vc[:, :S], vs[:, :S] = ref.kv_quantize_ref(v)


# ---------------------------------------------------------------------------------------
def _qkv_params(at):
    return [at.wq.weight, at.wk.weight, at.wv.weight]


def _prefill_attention(model, layer, n1, B: int, S: int, kc, vc, ks=None, vs=None):
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
    _store_prompt_kv(k, v, kc, vc, ks, vs)
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


def _check_cache(model, cache: KVCache, B: int):
    a = model.model_args
    if cache.batch != B or len(cache.k) != a.n_layers or tuple(cache.k[0].shape[2:]) != (a.kv_heads, a.head_dim):
        raise ValueError("KVCache does not match the model / batch")
    w = model.tok_embeddings.weight
    kind = getattr(cache, "fp8", False)
    dtype = cache.dtype if kind else cache.k[0].dtype
    if dtype != w.dtype or cache.k[0].device != w.device:
        raise ValueError(f"KVCache is {dtype} on {cache.k[0].device}, the model {w.dtype} on {w.device}")
    if kind and (cache.k[0].dtype != torch.uint8 or cache.k_scale[0] is None or
                 tuple(cache.k_scale[0].shape) != tuple(cache.k[0].shape[:-1])):
        raise ValueError("KVCache: an fp8 cache holds uint8 k / v and fp32 scales [B, capacity, Hkv]")


def _refuse_fp8(cache: KVCache, what: str) -> None:
    if getattr(cache, "fp8", False):
        raise ValueError(f"{what} does not serve an fp8 KV cache: the prompt's attention is defined as unquantized "
                         f"(prefill), and new tokens attending to their own dequantized keys would change that")


def _extend_layers(model, tokens: torch.Tensor, cache: KVCache):
    """tokens [B, T] through every layer as an append at ``cache.kv_len`` (left unchanged): per layer the QKV
    GEMM on [B * T, dim], the T-token ``rope_append``, ``attn_extend``, W_o and the MLP, with the rounding
    points of ``decode_step``. Returns (h, pending) [B, T, dim] for :func:`_head`."""
    B, T = tokens.shape
    a = model.model_args
    Hq, Hkv, D = a.n_heads, a.kv_heads, a.head_dim
    nq = Hq * D
    scale = 1.0 / math.sqrt(D)
    emb = model.tok_embeddings.weight
    h = F.embedding(tokens.contiguous(), emb, model._slot([emb]))
    pending = None
    for i, layer in enumerate(model.layers.values()):
        if pending is None:
            x, n1 = h, model._norm(layer.attention_norm, h, None)
        else:
            x, n1 = model._norm(layer.attention_norm, h, pending)
        at = layer.attention
        qkv = torch.mm(n1.reshape(B * T, n1.shape[-1]), model._weight(_qkv_params(at)).t())
        rope_append(qkv, model.rope_tab, cache.kv_len, cache.k[i], cache.v[i])
        o, _ = attention_extend(qkv[:, :nq].view(B, T, Hq, D), cache.k[i], cache.v[i], cache.kv_len, scale)
        att = F._mm_nt(o.view(B * T, nq), model._weight([at.wo.weight]), "o").view(B, T, -1)
        h, n2 = model._norm(layer.ffn_norm, x, att)
        pending = _mlp(model, layer, n2)
    return h, pending


@torch.no_grad()
def extend(model, tokens: torch.Tensor, n_new: torch.Tensor, cache: KVCache, return_all: bool = False) -> torch.Tensor:
    """Append ``n_new[b]`` tokens (``tokens`` [B, T] right-padded, 1 <= n_new[b] <= T, values outside are
    clamped) to every sequence at its own ``kv_len[b]`` -> logits [B, V] of row n_new[b] - 1, the next
    position's; ``kv_len += n_new`` (clamped at the capacity). A follow-up turn, a continuation after a
    shared prefix, one piece of a chunked prefill, the pass a speculative verifier needs.

    All T rows are computed: the pad rows' k / v land beyond the new ``kv_len`` and are overwritten by
    whatever is appended next, as prompt padding is in :func:`prefill`. A token whose position is at or
    beyond the capacity stores nothing and attends to the whole cache (T = 1 overwrites the last row, as
    ``decode_step`` does). ``n_new`` and ``kv_len`` stay on the device: no host synchronisation.
    ``return_all=True`` returns the logits of every row, [B, T, V], instead (scoring; pad rows included).
    fp8 caches are refused with ``ValueError``."""
    if tokens.dim() != 2 or tokens.shape[1] < 1:
        raise ValueError(f"extend: tokens must be [B, T] with T >= 1, got {tuple(tokens.shape)}")
    B, T = tokens.shape
    _check_cache(model, cache, B)
    _refuse_fp8(cache, "extend")
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
def prefill(model, tokens: torch.Tensor, lens: torch.Tensor, cache: KVCache, chunk: int = 0) -> torch.Tensor:
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
    piece would attend to dequantized keys. ``chunk = 0`` is the one-shot path."""
    B, S = tokens.shape
    _check_cache(model, cache, B)
    if S > cache.capacity:
        raise ValueError(f"prompt length {S} exceeds the cache capacity {cache.capacity}")
    lens = lens.to(device=tokens.device, dtype=torch.long)
    if chunk < 0:
        raise ValueError(f"prefill: chunk must be >= 0, got {chunk}")
    if chunk > 0:
        _refuse_fp8(cache, "prefill(chunk > 0)")
        return _prefill_chunked(model, tokens, lens, cache, int(chunk))
    emb = model.tok_embeddings.weight
    h = F.embedding(tokens, emb, model._slot([emb]))
    pending = None
    for i, layer in enumerate(model.layers.values()):
        if pending is None:
            x, n1 = h, model._norm(layer.attention_norm, h, None)
        else:
            x, n1 = model._norm(layer.attention_norm, h, pending)
        att = _prefill_attention(model, layer, n1, B, S, cache.k[i], cache.v[i], cache.k_scale[i], cache.v_scale[i])
        h, n2 = model._norm(layer.ffn_norm, x, att)
        pending = _mlp(model, layer, n2)
    cache.kv_len.copy_(lens.clamp(0, cache.capacity))
    rows = (lens - 1).clamp(0, S - 1)
    bi = torch.arange(B, device=tokens.device)
    return _head(model, h[bi, rows].contiguous(), None if pending is None else pending[bi, rows].contiguous())


@torch.no_grad()
def decode_step(model, tokens: torch.Tensor, cache: KVCache) -> torch.Tensor:
    """One token per sequence (tokens [B], the token at position kv_len[b]) -> logits [B, V] for the
    next position; kv_len grows by one (clamped at the capacity). No host synchronisation."""
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
    for i, layer in enumerate(model.layers.values()):
        if pending is None:
            x, n1 = h, model._norm(layer.attention_norm, h, None)
        else:
            x, n1 = model._norm(layer.attention_norm, h, pending)
        at = layer.attention
        qkv = torch.mm(n1, model._weight(_qkv_params(at)).t())
        ks, vs = cache.k_scale[i], cache.v_scale[i]  # None: a cache in the model's dtype
        rope_append(qkv, model.rope_tab, cache.kv_len, cache.k[i], cache.v[i], ks, vs)
        o, _ = attention_decode(qkv[:, :nq].view(B, Hq, D), cache.k[i], cache.v[i], att_len, scale, ks, vs)
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
             kv_cache_dtype: str = "model", prefill_chunk: int = 0) -> Tuple[List[List[int]], List[str]]:
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

    ``prefill_chunk=N`` (N > 0) feeds the prompt through :func:`prefill` in pieces of N columns, bounding the
    prefill's activation memory by B * N rows; the tokens are those of the one-shot prefill up to summation
    order. It needs the cache and refuses ``kv_cache_dtype="fp8"``. ``stats["prefill_chunks"]`` is the number
    of pieces (0: the one-shot prefill)."""
    if temperature < 0 or not 0.0 < top_p <= 1.0 or top_k < 0 or max_new_tokens < 1:
        raise ValueError("generate: need temperature >= 0, 0 < top_p <= 1, top_k >= 0, max_new_tokens >= 1")
    if sampler not in ("torch", "philox"):
        raise ValueError(f"generate: sampler must be 'torch' or 'philox', got {sampler!r}")
    if kv_cache_dtype not in KV_DTYPES:
        raise ValueError(f"generate: kv_cache_dtype must be one of {KV_DTYPES}, got {kv_cache_dtype!r}")
    if kv_cache_dtype != "model" and not use_cache:
        raise ValueError(f"generate: kv_cache_dtype={kv_cache_dtype!r} needs the KV cache (use_cache=True)")
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
    if use_cache:
        cache = KVCache(args, B, cap, dtype, device, kv_cache_dtype)
        logits = prefill(model, buf[:, :S], lens, cache, chunk=prefill_chunk)
    else:
        bi = torch.arange(B, device=device)
        logits = model(buf[:, :S])[bi, lens - 1]
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
