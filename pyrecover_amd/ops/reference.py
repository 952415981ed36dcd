"""Plain-PyTorch reference math for every fused op.

These functions reproduce the reference model's numerics (reference model.py) and are used
(1) as the fp32 oracle in the kernel tests and (2) as the implementation on CPU tensors (the
CPU/gloo configuration of BASELINE.json). They are never used for GPU tensors.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch
import torch.nn.functional as F


def precompute_freqs_cis(dim: int, end: int, theta: float = 10000.0) -> torch.Tensor:
    """complex64 [end, dim/2] rotation table, identical to reference model.py:52-72."""
    freqs = 1.0 / (theta ** (torch.arange(0, dim, 2)[: (dim // 2)].float() / dim))
    t = torch.arange(end, device=freqs.device)
    freqs = torch.outer(t, freqs).float()
    return torch.polar(torch.ones_like(freqs), freqs)


def rope_table(freqs_cis: torch.Tensor) -> torch.Tensor:
    """fp32 [S, D/2, 2] = (cos, sin), the layout the HIP RoPE kernel reads."""
    return torch.view_as_real(freqs_cis).contiguous()


def up(x: torch.Tensor) -> torch.Tensor:
    """Opmath of ``x``: fp32 for 16-bit/fp32 tensors, fp64 for fp64 (fp64 models stay fp64)."""
    return x.to(torch.promote_types(x.dtype, torch.float32))


# ---------------------------------------------------------------------------------------
def rmsnorm_ref(x: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
    """reference model.py:44-49"""
    xf = up(x)
    out = (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)).type_as(x)
    return out * w


def rmsnorm_fwd(x, delta, w, eps):
    """(h, y, rstd) with h = round(x + delta) when delta is given."""
    h = x if delta is None else (x + delta)
    hf = up(h)
    rstd = torch.rsqrt(hf.pow(2).mean(-1) + eps)
    y = (hf * rstd.unsqueeze(-1)).to(h.dtype) * w
    return h, y, rstd.reshape(-1)


def rmsnorm_bwd(dy, h, w, rstd, dres):
    """returns (dx, dw_fp32) with the same rounding points as the HIP kernel."""
    D = h.shape[-1]
    hf = up(h).reshape(-1, D)
    dyf = up(dy).reshape(-1, D)
    r = rstd.reshape(-1, 1)
    nb = up((hf * r).to(h.dtype))
    dw = (dyf * nb).sum(0)
    g = up((dyf * up(w)).to(h.dtype))
    dot = (g * hf).sum(-1, keepdim=True)
    dx = (r * (g - hf * (r * r * dot / D))).to(h.dtype)
    if dres is not None:
        dx = dx + dres.reshape(-1, D)
    return dx.reshape(h.shape), dw


def doc_positions(doc_start: torch.Tensor) -> torch.Tensor:
    """Packed sequences: int64 [B, S] position of each token within its document, i - doc_start[b, i]
    with doc_start clamped into [0, i] (as the HIP kernels clamp it)."""
    S = doc_start.shape[-1]
    i = torch.arange(S, device=doc_start.device)
    return i - torch.minimum(doc_start.long().clamp_min(0), i)


def doc_mask(doc_start: torch.Tensor) -> torch.Tensor:
    """bool [B, 1, S, S], True where query i may NOT see key j: visible iff doc_start[b, i] <= j <= i."""
    S = doc_start.shape[-1]
    i = torch.arange(S, device=doc_start.device)
    lo = torch.minimum(doc_start.long().clamp_min(0), i)  # [B, S]
    j = i.view(1, 1, S)
    return ((j > i.view(1, S, 1)) | (j < lo.unsqueeze(-1))).unsqueeze(1)


def rope_inplace_2d(x2d: torch.Tensor, ncols: int, tab: torch.Tensor, head_dim: int, seq_len: int,
                    inverse: bool = False, doc_start: Optional[torch.Tensor] = None):
    """Rotate the first `ncols` columns of every row (heads of size head_dim), interleaved pairs.
    doc_start ([B, S], packed sequences): token i of a row takes table row i - doc_start[b, i]."""
    T = x2d.shape[0]
    v = up(x2d[:, :ncols]).reshape(T // seq_len, seq_len, ncols // head_dim, head_dim // 2, 2)
    if doc_start is not None:
        rows = tab[doc_positions(doc_start.reshape(T // seq_len, seq_len))].to(v.dtype)  # [B, S, D/2, 2]
        c, s = rows[..., 0].unsqueeze(2), rows[..., 1].unsqueeze(2)
    else:
        c = tab[:seq_len, :, 0].view(1, seq_len, 1, head_dim // 2)
        s = tab[:seq_len, :, 1].view(1, seq_len, 1, head_dim // 2)
    if inverse:
        s = -s
    a, b = v[..., 0], v[..., 1]
    out = torch.stack([a * c - b * s, a * s + b * c], dim=-1)
    x2d[:, :ncols] = out.reshape(T, ncols).to(x2d.dtype)


def apply_rotary_emb_ref(xq, xk, freqs_cis):
    """reference model.py:101-127 ([B, S, H, D] tensors)"""
    xq_ = torch.view_as_complex(up(xq).reshape(*xq.shape[:-1], -1, 2))
    xk_ = torch.view_as_complex(up(xk).reshape(*xk.shape[:-1], -1, 2))
    fc = freqs_cis[: xq.shape[1]].view(1, xq.shape[1], 1, xq_.shape[-1])
    xq_out = torch.view_as_real(xq_ * fc).flatten(3)
    xk_out = torch.view_as_real(xk_ * fc).flatten(3)
    return xq_out.type_as(xq), xk_out.type_as(xk)


def attention_ref(q, k, v, causal: bool = True, scale: Optional[float] = None,
                  doc_start: Optional[torch.Tensor] = None):
    """[B, S, H, D] in/out; GQA by repeating kv heads (reference model.py:130-139, 217-229).
    doc_start ([B, S], packed sequences): causal within each document only."""
    B, S, Hq, D = q.shape
    Hkv = k.shape[2]
    if Hkv != Hq:
        k = k.repeat_interleave(Hq // Hkv, dim=2)
        v = v.repeat_interleave(Hq // Hkv, dim=2)
    if doc_start is not None:
        o = F.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2),
                                           attn_mask=~doc_mask(doc_start), scale=scale)
        return o.transpose(1, 2).contiguous()
    o = F.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2),
                                       is_causal=causal, scale=scale)
    return o.transpose(1, 2).contiguous()


def attention_lse_ref(q, k, v, causal=True, scale=None, doc_start=None):
    """fp32 attention output + natural-log LSE [B, H, S] (oracle for the HIP kernel)."""
    B, S, Hq, D = q.shape
    Hkv = k.shape[2]
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    kk = up(k).repeat_interleave(Hq // Hkv, dim=2)
    vv = up(v).repeat_interleave(Hq // Hkv, dim=2)
    s = torch.einsum("bqhd,bkhd->bhqk", up(q), kk) * scale
    if doc_start is not None:
        s = s.masked_fill(doc_mask(doc_start), float("-inf"))
    elif causal:
        m = torch.ones(S, S, dtype=torch.bool, device=q.device).triu(1)
        s = s.masked_fill(m, float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    p = torch.softmax(s, dim=-1)
    o = torch.einsum("bhqk,bkhd->bqhd", p, vv)
    return o, lse


def swiglu_ref(g, u):
    """reference model.py:269: silu(w1 x) * w3 x"""
    return F.silu(g) * u


def swiglu_bwd_ref(dy, g, u):
    gf, uf, dyf = up(g), up(u), up(dy)
    sg = torch.sigmoid(gf)
    a = up((gf * sg).to(g.dtype))
    da = up((dyf * uf).to(g.dtype))
    du = dyf * a
    dg = da * sg * (1 + gf * (1 - sg))
    return dg.to(g.dtype), du.to(g.dtype)


def cross_entropy_ref(logits, labels, ignore_index: int = -100):
    """reference train.py:253,263-266: sum-reduced CE on fp32 logits / #non-ignored labels."""
    n = labels.ne(ignore_index).sum()
    loss = F.cross_entropy(up(logits.flatten(0, -2)), labels.flatten(), reduction="sum",
                           ignore_index=ignore_index)
    return loss / n


def cross_entropy_reg_ref(logits, labels, ignore_index: int = -100, z_loss: float = 0.0, label_smoothing: float = 0.0):
    """The regularised objective and its statistics in torch math (the opmath of ``logits``).

    Per valid row (label in [0, V) and not ``ignore_index``), lse = logsumexp(x): nll = lse - x[label],
    smooth = lse - mean(x), zterm = z_loss * lse^2. With n valid rows,
    objective = ((1 - eps) * sum nll + eps * sum smooth + sum zterm) / n, which at z_loss = 0 is
    ``F.cross_entropy(label_smoothing=eps, reduction="sum") / n``.

    Returns (objective, stats): stats [8] = {objective, n, sum nll / n (the plain cross-entropy),
    sum zterm / n, sum smooth / n, mean lse, max |lse| (both over the valid rows), 0}. As in the HIP
    kernels, sum smooth / n is only formed with label_smoothing > 0 (else that entry is 0, NaN for
    n = 0). Differentiable through ``objective``; stats is detached."""
    x = up(logits.flatten(0, -2))
    lab = labels.flatten()
    V = x.shape[-1]
    valid = lab.ne(ignore_index) & lab.ge(0) & lab.lt(V)
    n = valid.sum()
    nf = n.to(x.dtype)
    lse = torch.logsumexp(x, dim=-1)
    zero = torch.zeros_like(lse)
    nll = torch.where(valid, lse - x.gather(1, lab.clamp(0, V - 1)[:, None])[:, 0], zero)
    lv = torch.where(valid, lse, zero)
    ce = nll.sum() / nf
    zt = z_loss * (lv.pow(2).sum() / nf)
    if label_smoothing > 0:
        sv = torch.where(valid, lse - x.mean(-1), zero).sum() / nf
    else:
        sv = zero.sum() / nf
    obj = (1.0 - label_smoothing) * ce + label_smoothing * sv + zt
    with torch.no_grad():
        stats = torch.stack([obj, nf, ce, zt, sv, lv.sum() / nf, lv.abs().max() if lv.numel() else zero.sum(),
                             torch.zeros_like(nf)]).detach()
    return obj, stats


# ---------------------------------------------------------------------------------------
# KV-cache generation (pyrecover_amd/inference.py; HIP: csrc/kernels/attention_decode.hip)
def attention_decode_ref(q, k_cache, v_cache, kv_len, scale: Optional[float] = None):
    """One query per sequence over a KV cache, in the input's precision promoted to at least fp32.

    q [B, Hq, D]; k_cache, v_cache [B, cap, Hkv, D]; kv_len integer [B] (clamped into [0, cap]):
    sequence b attends to keys 0 .. kv_len[b] - 1, and whatever the caches hold beyond that (NaN and
    Inf included) never reaches the output. Returns (o [B, Hq, D] in that precision, lse [B, Hq]);
    length 0 gives o = 0 and lse = -inf."""
    B, Hq, D = q.shape
    cap, Hkv = k_cache.shape[1], k_cache.shape[2]
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    n = kv_len.to(device=q.device, dtype=torch.long).clamp(0, cap)
    dead = torch.arange(cap, device=q.device).view(1, cap) >= n.view(B, 1)  # [B, cap]
    qg = up(q).view(B, Hkv, Hq // Hkv, D)
    kk, vv = up(k_cache), up(v_cache).masked_fill(dead.view(B, cap, 1, 1), 0)
    s = torch.einsum("bhgd,bkhd->bhgk", qg, kk) * scale
    s = s.masked_fill(dead.view(B, 1, 1, cap), float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse.clamp_min(torch.finfo(s.dtype).min).unsqueeze(-1))  # an empty row: exp(-inf) = 0
    o = torch.einsum("bhgk,bkhd->bhgd", p, vv)
    return o.reshape(B, Hq, D), lse.reshape(B, Hq)


def attention_extend_ref(q, k_cache, v_cache, kv_len, scale: Optional[float] = None):
    """T new queries per sequence over a KV cache that already holds their own k / v, in the input's
    precision promoted to at least fp32 (HIP: csrc/kernels/attention_extend.hip).

    q [B, T, Hq, D]; k_cache, v_cache [B, cap, Hkv, D]; kv_len integer [B], the tokens held BEFORE this
    append (clamped into [0, cap]): query t of sequence b sits at position p = kv_len[b] + t and attends
    to keys 0 .. min(p, cap - 1), so every row sees at least key 0. Whatever the caches hold beyond a
    row's bound (NaN and Inf included) never reaches its output. Returns (o [B, T, Hq, D] in that
    precision, lse [B, T, Hq])."""
    B, T, Hq, D = q.shape
    cap, Hkv = k_cache.shape[1], k_cache.shape[2]
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    n = kv_len.to(device=q.device, dtype=torch.long).clamp(0, cap)
    last = (n.view(B, 1) + torch.arange(T, device=q.device).view(1, T)).clamp(max=cap - 1)  # [B, T]
    dead = torch.arange(cap, device=q.device).view(1, 1, cap) > last.unsqueeze(-1)  # [B, T, cap]
    unseen = dead.all(dim=1)  # [B, cap]: keys no row of the sequence sees
    qg = up(q).view(B, T, Hkv, Hq // Hkv, D)
    kk = up(k_cache).masked_fill(unseen.view(B, cap, 1, 1), 0)
    vv = up(v_cache).masked_fill(unseen.view(B, cap, 1, 1), 0)
    s = torch.einsum("bthgd,bkhd->bthgk", qg, kk) * scale
    s = s.masked_fill(dead.view(B, T, 1, 1, cap), float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse.unsqueeze(-1))
    o = torch.einsum("bthgk,bkhd->bthgd", p, vv)
    return o.reshape(B, T, Hq, D), lse.reshape(B, T, Hq)


def rope_append_ref(qkv, tab, kv_len, k_cache, v_cache) -> None:
    """The fused QKV rows [B * T, (Hq + 2 Hkv) D] of T new tokens per sequence (B is the caches'), row
    b * T + t at position p = clamp(kv_len[b], 0, cap) + t: q is rotated in place, the rotated k and the
    plain v are written into row p of the caches (RoPE math of :func:`rope_inplace_2d`: opmath rotation
    from table row p, one rounding). T = 1 clamps the row into the cache, pos[b] = clamp(kv_len[b], 0,
    cap - 1); with T > 1 a row with p >= cap stores nothing and its q takes table row cap - 1."""
    bi, pos, k, v = _rope_new_rows(qkv, tab, kv_len, *k_cache.shape)
    k_cache[bi, pos] = k
    v_cache[bi, pos] = v


def _rope_new_rows(qkv, tab, kv_len, B: int, cap: int, Hkv: int, D: int):
    """Rotates q in place; returns, for the rows that are stored, (batch index, pos, rotated k [n, Hkv, D] in
    qkv's dtype, v [n, Hkv, D])."""
    N = qkv.shape[0]
    T = N // B
    nk = Hkv * D
    nq = qkv.shape[1] - 2 * nk
    at = (kv_len.to(device=qkv.device, dtype=torch.long).clamp(0, cap).view(B, 1) +
          torch.arange(T, device=qkv.device).view(1, T)).reshape(N)
    pos = at.clamp(max=cap - 1)
    rows = tab[pos].to(up(qkv).dtype)  # [N, D/2, 2]
    c, s = rows[..., 0].unsqueeze(1), rows[..., 1].unsqueeze(1)
    x = up(qkv[:, :nq + nk]).reshape(N, (nq + nk) // D, D // 2, 2)
    a, b = x[..., 0], x[..., 1]
    rot = torch.stack([a * c - b * s, a * s + b * c], dim=-1).reshape(N, nq + nk).to(qkv.dtype)
    qkv[:, :nq] = rot[:, :nq]
    bi = torch.arange(B, device=qkv.device).repeat_interleave(T)
    k, v = rot[:, nq:].view(N, Hkv, D), qkv[:, nq + nk:].view(N, Hkv, D)
    if T == 1:
        return bi, pos, k, v
    keep = at < cap  # a data-dependent selection: the torch path may synchronise, the HIP kernel does not
    return bi[keep], pos[keep], k[keep], v[keep]


# ---------------------------------------------------------------------------------------
# fp8 KV cache (HIP: csrc/kernels/attention_decode_fp8.hip). A cache row, the D values of one (sequence,
# position, kv head), is D bytes of OCP e4m3fn (held as uint8) and one fp32 scale 2^e.

def kv_quantize_ref(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """x [..., D] -> (bytes uint8 [..., D], scale fp32 [...]) by the cache's rule, on x cast to fp32 (exact
    for bf16 / fp16): amax = max |x_i|; amax == 0 gives scale 1 and bytes 0; otherwise (m, k) = frexp(amax)
    and e = clamp(k - 9 + (m > 0.875), -126, 127), the smallest e with amax * 2^-e <= 448; scale = 2^e and
    byte_i = e4m3fn_rne(x_i * 2^-e). The product is exact, so there is one rounding and no saturation."""
    xf = x.float()
    amax = xf.abs().amax(dim=-1)
    m, k = torch.frexp(amax)
    e = (k.to(torch.int32) - 9 + (m > 0.875).to(torch.int32)).clamp(-126, 127)
    e = torch.where(amax == 0, torch.zeros_like(e), e)
    y = torch.ldexp(xf, -e.unsqueeze(-1)).masked_fill((amax == 0).unsqueeze(-1), 0.0)  # -0.0 rows: bytes 0 too
    return y.to(torch.float8_e4m3fn).view(torch.uint8), torch.ldexp(torch.ones_like(amax), e)


def kv_dequantize_ref(q: torch.Tensor, scale: torch.Tensor, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """bytes [..., D], scale [...] -> byte_i * scale in ``dtype``: exact in fp32, bf16 and fp16."""
    return (q.view(torch.float8_e4m3fn).to(torch.float32) * scale.unsqueeze(-1)).to(dtype)


def rope_append_fp8_ref(qkv, tab, kv_len, k_cache, v_cache, k_scale, v_scale) -> None:
    """:func:`rope_append_ref` over an fp8 cache: q is rotated in place as there; the k row is rotated in
    opmath, rounded once to qkv's dtype and then quantized, the v row quantized from its values: the cache
    is a pure function of what the 16-bit cache would hold."""
    bi, pos, k, v = _rope_new_rows(qkv, tab, kv_len, *k_cache.shape)
    k_cache[bi, pos], k_scale[bi, pos] = kv_quantize_ref(k)
    v_cache[bi, pos], v_scale[bi, pos] = kv_quantize_ref(v)


def attention_decode_fp8_ref(q, k_cache, v_cache, k_scale, v_scale, kv_len, scale: Optional[float] = None):
    """:func:`attention_decode_ref` on the dequantized cache, in q's precision promoted to at least fp32."""
    dt = up(q).dtype
    return attention_decode_ref(q, kv_dequantize_ref(k_cache, k_scale, dt), kv_dequantize_ref(v_cache, v_scale, dt),
                                kv_len, scale)


# ---------------------------------------------------------------------------------------
# Sampling (pyrecover_amd/inference.py; HIP: csrc/kernels/sample.hip)
SAMPLE_STREAM = 3  # Philox counter word 3: after the stochastic-rounding streams 0, 1, 2 (optim/sr.py)


def sample_uniform(pos: torch.Tensor, seed: int) -> torch.Tensor:
    """The uniform in [0, 1) of the draw of row b at absolute position pos[b] (fp64, exact):
    ``(philox4x32_10((b, pos[b], 0, 3), seed)[0] >> 8) * 2^-24``. A pure function of (seed, row, position)."""
    from ..optim.sr import philox4x32_10

    pos = torch.as_tensor(pos).to(torch.int64).reshape(-1)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    rows = torch.arange(pos.numel(), device=pos.device)
    w0 = philox4x32_10((rows, pos & 0xFFFFFFFF, 0, SAMPLE_STREAM), (seed & 0xFFFFFFFF, seed >> 32))[0]
    return (w0 >> 8).to(torch.float64) * 2.0 ** -24


def greedy_total_order(logits: torch.Tensor) -> torch.Tensor:
    """The lowest id holding the row maximum under NaN < -inf < finite < +inf. On rows without a NaN this
    is ``inference.greedy_token``."""
    V = logits.shape[-1]
    nan = torch.isnan(logits)
    xs = logits.masked_fill(nan, float("-inf"))
    top = xs.max(dim=-1, keepdim=True).values
    holds = (xs == top) & (~nan | nan.all(dim=-1, keepdim=True))
    ids = torch.arange(V, device=logits.device).expand_as(logits)
    return torch.where(holds, ids, V).min(dim=-1).values.clamp_(max=V - 1)


def sample_philox_ref(logits: torch.Tensor, pos, temperature: float, top_k: int = 0, top_p: float = 1.0,
                      seed: int = 0) -> torch.Tensor:
    """Token ids [B] from logits [B, V] by the rule of csrc/kernels/sample.hip, in torch (opmath: the
    input's precision promoted to at least fp32): the CPU path, the path of fp32 / fp64 logits on the GPU.

    Tokens are ranked by z = x / T descending, ties by ascending id (a stable sort). top-k keeps every
    token with z >= the k-th largest z. top-p keeps the shortest prefix of the ranking whose softmax mass
    over the top-k survivors reaches top_p (a token is dropped iff the mass ranked above it is >= top_p;
    the first always stays). The draw is the first kept token whose cumulative mass exceeds
    u * (kept mass), the last kept token if rounding leaves none, u = sample_uniform(pos, seed)[b].
    A row whose maximum is not finite, and ``temperature == 0`` (no Philox call), give
    :func:`greedy_total_order`."""
    if temperature < 0 or not 0.0 < top_p <= 1.0 or top_k < 0:
        raise ValueError("sample_philox_ref: need temperature >= 0, 0 < top_p <= 1, top_k >= 0")
    x = up(logits)
    B, V = x.shape
    first = greedy_total_order(x)
    if temperature == 0.0:
        return first
    u = sample_uniform(torch.as_tensor(pos).to(x.device), seed).to(x.dtype)
    xs = x.masked_fill(torch.isnan(x), float("-inf"))
    sz, si = torch.sort(xs / temperature, dim=-1, descending=True, stable=True)
    keep = torch.ones_like(sz, dtype=torch.bool)
    if 0 < top_k < V:
        keep = sz >= sz[:, top_k - 1:top_k]
    finite = torch.isfinite(sz[:, 0])
    w = torch.exp(sz - sz[:, :1].masked_fill(~finite[:, None], 0.0))
    w = torch.where(keep & torch.isfinite(w), w, torch.zeros_like(w))
    zero = torch.zeros(B, 1, dtype=w.dtype, device=w.device)
    if top_p < 1.0:
        cum = torch.cumsum(w, dim=-1)
        before = torch.cat([zero, cum[:, :-1]], dim=-1)
        drop = before >= top_p * cum[:, -1:]
        drop[:, 0] = False
        keep = keep & ~drop
        w = torch.where(keep, w, torch.zeros_like(w))
    cum = torch.cumsum(w, dim=-1)
    rank = torch.arange(V, device=x.device).expand(B, V)
    hit = keep & (cum > u[:, None] * cum[:, -1:])
    idx = torch.where(hit, rank, V).min(dim=-1).values
    last = torch.where(keep, rank, -1).max(dim=-1).values
    idx = torch.where(idx < V, idx, last)
    tok = si.gather(1, idx[:, None])[:, 0]
    return torch.where(finite, tok, first)
