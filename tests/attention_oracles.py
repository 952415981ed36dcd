"""fp64 oracle, abs-oracle (error scale), rounding baseline with seeded defects, and input recipes for
the attention kernels.

Shared by tests/test_attention_rowerr_gpu.py (HIP kernels against the oracle, on the GPU) and
tests/test_attention_oracles.py (oracle against fp64 autograd, baseline and seeded defects against the
same cap, on the CPU), so a recipe and the cap are validated before a kernel sees them. Everything here
is device-agnostic torch and works one kv-head group at a time.

Oracle      fp64 math on the upcast inputs, no intermediate rounding. forward_oracle gives (o, lse);
            backward_oracle takes o and lse as inputs, as the kernels do (delta = rowsum(dO * O),
            P = exp(S - lse)), and gives (dq, dk, dv), optionally with the inverse RoPE of
            reference.rope_inplace_2d(..., inverse=True) on dq and dk.
Abs-oracle  the same computation with every operand replaced by its absolute value (no cancellation):
            M_o = |P| |V|, |dS|+ = |P| (|dO| |V|^T + rowsum(|dO| |O|)), M_dq = scale |dS|+ |K|,
            M_dk = scale |dS|+^T |Q|, M_dv = |P|^T |dO|. Masked positions contribute 0. fp16 rounds with
            fl(x) = x (1 + e) + h, |e| <= u, |h| <= 2^-24 (the subnormal spacing: P and dS flush below
            it), so every unmasked |P| and |dS|+ element gets the absolute underflow term 2^-24 / u:
            divided by u because the cap multiplies M_r by u. (Adding a bare 2^-24 leaves an error of
            2^-25 |dO| against a scale of 2^-24 |dO| on a key that no query attends to: rho = 0.5 on an
            honest fp16 emulation, measured 259 u on `peaked`.) bf16 has fp32's exponent range: no term.
Metric      rho = max over rows (the D-vector at one (b, s, h)) of |got_r - oracle_r|_2 / |M_r|_2; the
            row L2 norm is invariant under the RoPE rotation.
Cap         rho <= (n_round + 1) u, u = 2^-(mantissa bits + 1): each 16-bit rounding on the path to an
            output adds at most u M_r to first order; the extra u covers v_exp_f32, fp32 accumulation
            and ties that land on the other side. N_ROUND below lists the roundings with file:line.
            fp32 kernels: rho <= min(4 * measured, 2^-16) (the project's fp32 rule, kernel_oracles.py).
lse         max|lse - oracle| <= 4 * (error of torch.logsumexp over fp32 q k^T scale) + 4 ulp_fp32(max|score|).
Baseline    torch emulation, fp32 opmath, tiled online softmax over 64-key tiles, rounding exactly where
            N_ROUND says the kernels round; `mutation=` seeds one of MUTATIONS.
"""
import functools
import math

import torch

KT = 64  # key tile of the forward kernels (baseline tiling, stair recipe)
MANT_BITS = {torch.bfloat16: 7, torch.float16: 10, torch.float32: 23}
FP32_CAP = 2.0 ** -16
FP16_FLUSH = 2.0 ** -24
LOG2E = 1.4426950408889634

# 16-bit roundings on the path to each output (the kernels scale the fp32 scores; no operand is pre-multiplied),
# final store included.
#   o   P -> T before P V          attention.hip:189 (fwd_kernel), :403 / :422 (fwd_p_kernel), attention_docs.hip:158
#       final store                attention.hip:215, :483, attention_docs.hip:182 (attn_common.h:74 pack_x2)
#   dq  dS -> T before dS K        attention.hip:1300 (bwd_dq_kernel; :1253 / :1264 pipelined), attention_docs.hip:298,
#                                  attention_bwd_fused.hip:217 (through the LDS dS image)
#       final store                attention.hip:1319, attention_docs.hip:317, attention_bwd_fused.hip:275
#   dk  dS -> T before dS^T Q      attention.hip:668 (two-wave), :819 (ring), :1014 / :1025 (pipelined),
#                                  attention_bwd_fused.hip:217, attention_docs.hip:453
#       final store                attention.hip:687, :841, :1044, :1069 (split reduce),
#                                  attention_bwd_fused.hip:288, attention_docs.hip:472
#   dv  P -> T before P^T dO       the same lines as dk's dS
#       final store                attention.hip:689, :843, :1045, :1069, attention_bwd_fused.hip:290,
#                                  attention_docs.hip:474
#   decode o: P and the partial sums stay fp32 (attention_decode.hip:217-246); the one rounding is the
#       final store, attention_decode.hip:309
# Not a rounding of the u M_r kind, and so not countable: K c -> T with c = scale log2(e), which the 8-wave,
# ring, pipelined and fused dK/dV kernels once applied so that P = exp2(S') needed no multiply. It moves every
# score by up to u scale sum|q_d||k_d|, and exp turns that into a relative error of P that grows with the
# size of the scores (dv 12-25 u on scores of tens of nats). Those kernels now scale the fp32 score;
# baseline(k_prescale=True) keeps the emulation, and test_attention_oracles.py shows it beyond the cap.
N_ROUND = {"o": 2, "dq": 2, "dk": 2, "dv": 2, "decode_o": 1}

MUTATIONS = ("lse_shift", "delta_zero_tail", "last_key_zero", "causal_off_by_one", "dq_no_scale",
             "dk_scale_twice", "gqa_modulo", "skip_rescale", "doc_boundary_ignored")

RECIPES = ("flat", "peaked", "peaked_rsqrt", "stair5", "stair9", "all_negative", "all_large", "spike_rows",
           "odd_scale")


def unit(dtype) -> float:
    """Storage rounding unit u = 2^-(mantissa bits + 1)."""
    return 2.0 ** -(MANT_BITS[dtype] + 1)


def cap(dtype, out: str) -> float:
    return (N_ROUND[out] + 1) * unit(dtype)


def dname(dtype) -> str:
    return str(dtype).replace("torch.", "")


# ------------------------------------------------------------------------------------------------
# masks: vis [B, Sq, Sk] bool, True where the query sees the key
def visibility(B, Sq, Sk, causal, doc_start=None, kv_len=None, shift=0, device="cpu"):
    i = torch.arange(Sq, device=device).view(1, Sq, 1)
    j = torch.arange(Sk, device=device).view(1, 1, Sk)
    vis = torch.ones(B, Sq, Sk, dtype=torch.bool, device=device)
    if causal or doc_start is not None:
        vis = vis & (j <= i + shift)
    if doc_start is not None:
        lo = torch.minimum(doc_start.long().clamp_min(0), torch.arange(Sq, device=device))  # as the kernels clamp
        vis = vis & (j >= lo.view(B, Sq, 1))
    if kv_len is not None:
        vis = vis & (j < kv_len.long().view(B, 1, 1))
    return vis


def _groups(Hq, Hkv, modulo=False):
    """(query heads, kv head) per group; modulo = the seeded defect kv head = hq % Hkv."""
    if modulo:
        return [(list(range(h, Hq, Hkv)), h) for h in range(Hkv)]
    rep = Hq // Hkv
    return [(list(range(h * rep, (h + 1) * rep)), h) for h in range(Hkv)]


def _scores(qg, kh, scale, vis):
    s = torch.einsum("bqrd,bkd->brqk", qg, kh) * scale
    return s.masked_fill(~vis[:, None], float("-inf"))


# ------------------------------------------------------------------------------------------------
# oracle
def forward_oracle(q, k, v, scale, vis):
    """fp64 (o [B, Sq, Hq, D], lse [B, Hq, Sq]); an all-masked row gives o = 0, lse = -inf."""
    B, Sq, Hq, D = q.shape
    Hkv = k.shape[2]
    o = torch.empty(B, Sq, Hq, D, dtype=torch.float64, device=q.device)
    lse = torch.empty(B, Hq, Sq, dtype=torch.float64, device=q.device)
    for hs, h in _groups(Hq, Hkv):
        s = _scores(q[:, :, hs].double(), k[:, :, h].double(), scale, vis)
        l = torch.logsumexp(s, dim=-1)
        p = torch.exp(s - l.clamp_min(-1e300)[..., None])
        o[:, :, hs] = torch.einsum("brqk,bkd->bqrd", p, v[:, :, h].double())
        lse[:, hs] = l
    return o, lse


def rope_inverse64(x, tab, doc_start=None):
    """x [B, S, H, D] fp64 with the inverse rotation of reference.rope_inplace_2d(inverse=True): pairs
    (2i, 2i + 1), (a + ib)(c - is); table row = position (restarting per document when packed)."""
    B, S, H, D = x.shape
    if doc_start is not None:
        i = torch.arange(S, device=x.device)
        pos = i - torch.minimum(doc_start.long().clamp_min(0), i)
        rows = tab[pos].double()  # [B, S, D/2, 2]
    else:
        rows = tab[:S].double().unsqueeze(0)
    c, s = rows[..., 0].unsqueeze(2), -rows[..., 1].unsqueeze(2)
    xv = x.reshape(B, S, H, D // 2, 2)
    a, b = xv[..., 0], xv[..., 1]
    return torch.stack([a * c - b * s, a * s + b * c], dim=-1).reshape(B, S, H, D)


def backward_oracle(q, k, v, o, lse, do, scale, vis, rope_tab=None, doc_start=None):
    """fp64 (dq, dk, dv) from the given o (delta) and lse (P), as the kernels compute them."""
    B, S, Hq, D = q.shape
    Hkv = k.shape[2]
    dq = torch.empty(B, S, Hq, D, dtype=torch.float64, device=q.device)
    dk = torch.empty(B, S, Hkv, D, dtype=torch.float64, device=q.device)
    dv = torch.empty_like(dk)
    for hs, h in _groups(Hq, Hkv):
        qg, kh, vh = q[:, :, hs].double(), k[:, :, h].double(), v[:, :, h].double()
        dog, og = do[:, :, hs].double(), o[:, :, hs].double()
        p = torch.exp(_scores(qg, kh, scale, vis) - lse[:, hs].double()[..., None])
        dp = torch.einsum("bqrd,bkd->brqk", dog, vh)
        delta = (dog * og).sum(-1).permute(0, 2, 1)  # [B, rep, S]
        ds = p * (dp - delta[..., None])
        dq[:, :, hs] = scale * torch.einsum("brqk,bkd->bqrd", ds, kh)
        dk[:, :, h] = scale * torch.einsum("brqk,bqrd->bkd", ds, qg)
        dv[:, :, h] = torch.einsum("brqk,bqrd->bkd", p, dog)
    if rope_tab is not None:
        dq, dk = rope_inverse64(dq, rope_tab, doc_start), rope_inverse64(dk, rope_tab, doc_start)
    return dq, dk, dv


def abs_oracle(q, k, v, o, lse, do, scale, vis, dtype):
    """Error scales (M_o, M_dq, M_dk, M_dv), fp64; do = None gives M_o alone (decode)."""
    B, Sq, Hq, D = q.shape
    Hkv = k.shape[2]
    flush = FP16_FLUSH / unit(dtype) if dtype == torch.float16 else 0.0  # absolute error in units of u (docstring)
    m_o = torch.empty(B, Sq, Hq, D, dtype=torch.float64, device=q.device)
    m_dq = torch.empty_like(m_o)
    m_dk = torch.empty(B, k.shape[1], Hkv, D, dtype=torch.float64, device=q.device)
    m_dv = torch.empty_like(m_dk)
    visf = vis[:, None].double()
    for hs, h in _groups(Hq, Hkv):
        qg, kh, vh = q[:, :, hs].double(), k[:, :, h].double().abs(), v[:, :, h].double().abs()
        p = torch.exp(_scores(qg, k[:, :, h].double(), scale, vis) - lse[:, hs].double().clamp_min(-1e300)[..., None])
        p = (p + flush) * visf
        m_o[:, :, hs] = torch.einsum("brqk,bkd->bqrd", p, vh)
        if do is None:
            continue
        dog, og = do[:, :, hs].double().abs(), o[:, :, hs].double().abs()
        dp = torch.einsum("bqrd,bkd->brqk", dog, vh)
        delta = (dog * og).sum(-1).permute(0, 2, 1)
        ds = (p * (dp + delta[..., None]) + flush) * visf
        m_dq[:, :, hs] = scale * torch.einsum("brqk,bkd->bqrd", ds, kh)
        m_dk[:, :, h] = scale * torch.einsum("brqk,bqrd->bkd", ds, qg.abs())
        m_dv[:, :, h] = torch.einsum("brqk,bqrd->bkd", p, dog)
    return (m_o,) if do is None else (m_o, m_dq, m_dk, m_dv)


def rho(got, want, m):
    """(max over rows of |got_r - want_r|_2 / |M_r|_2, flat index of that row)."""
    D = want.shape[-1]
    e = (got.double() - want.double()).reshape(-1, D).norm(dim=-1)
    s = m.double().reshape(-1, D).norm(dim=-1)
    assert bool((s > 0).all()), "abs-oracle row of norm 0"
    r = e / s
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    i = int(r.argmax())
    return float(r[i]), i


def fits_fp32(smax: float) -> bool:
    """A case fits the fp32 rule when four roundings of its largest score in the kernels' log2 domain stay
    inside the 2^-16 cap: 4 ulp_fp32(max|score| log2 e) <= 2^-16, i.e. max|score| < 64 / log2(e) = 44 nats
    (a score of 140 nats carries 1.5e-5 = 2^-16 of absolute error per fp32 rounding, and exp turns that
    into relative error of P in any fp32 implementation)."""
    return 4.0 * ulp32(smax * 1.4426950408889634) <= FP32_CAP


def ulp32(x: float) -> float:
    return 0.0 if x <= 0 else 2.0 ** (math.floor(math.log2(x)) - 23)


def lse_bound(q, k, scale, vis, lse64):
    """(4 * |torch.logsumexp(fp32 q k^T scale) - oracle| + 4 ulp_fp32(max |score|), max |score|)."""
    Hq, Hkv = q.shape[2], k.shape[2]
    base_err, smax = 0.0, 0.0
    for hs, h in _groups(Hq, Hkv):
        s = _scores(q[:, :, hs].float(), k[:, :, h].float(), scale, vis)
        fin = torch.isfinite(lse64[:, hs])
        d = (torch.logsumexp(s, dim=-1).double() - lse64[:, hs])[fin].abs()
        base_err = max(base_err, float(d.max()) if d.numel() else 0.0)
        smax = max(smax, float(s[torch.isfinite(s)].abs().max()))
    return 4.0 * base_err + 4.0 * ulp32(smax), smax


# ------------------------------------------------------------------------------------------------
# baseline: fp32 opmath, rounding where N_ROUND says, seeded defects
def _rt(x, dtype):
    return x.to(dtype).float()


def baseline(q, k, v, do, scale, causal, dtype, doc_start=None, rope_tab=None, mutation=None, o_lse=None,
             k_prescale=False):
    """(o, lse, dq, dk, dv): o, dq, dk, dv hold storage-dtype values (fp32 tensors), lse fp32. The backward
    runs on o_lse = (o, lse) when given (oracle-made inputs), else on the baseline's own forward.
    k_prescale: the backward forms P from K * scale * log2(e) rounded to the storage dtype, the defect the
    8-wave, ring, pipelined and fused dK/dV kernels had (N_ROUND)."""
    assert mutation is None or mutation in MUTATIONS, mutation
    B, S, Hq, D = q.shape
    Hkv = k.shape[2]
    ds_in = doc_start
    if mutation == "doc_boundary_ignored":
        assert doc_start is not None
        first = int(doc_start[0][doc_start[0] > 0].min())  # start of the second document of sequence 0
        ds_in = doc_start.clone()
        ds_in[0][doc_start[0] == first] = 0
    vis = visibility(B, S, S, causal, ds_in, shift=1 if mutation == "causal_off_by_one" else 0, device=q.device)
    groups = _groups(Hq, Hkv, modulo=mutation == "gqa_modulo")
    o = torch.empty(B, S, Hq, D)
    lse = torch.empty(B, Hq, S)
    for hs, h in groups:  # tiled online softmax, P rounded per tile relative to the running max
        qg, kh, vh = q[:, :, hs].float(), k[:, :, h].float(), v[:, :, h].float()
        s = _scores(qg, kh, scale, vis)
        m = torch.full(s.shape[:-1], float("-inf"))
        l = torch.zeros_like(m)
        acc = torch.zeros(B, len(hs), S, D)
        skipped = False
        for t in range(0, S, KT):
            st = s[..., t:t + KT]
            m_new = torch.maximum(m, st.max(-1).values)
            m_safe = m_new.clamp_min(-1e30)
            alpha = torch.exp(m.clamp_min(-1e30) - m_safe)
            p = torch.exp(st - m_safe[..., None])
            l = l * alpha + p.sum(-1)
            grew = (m_new > m) & torch.isfinite(m)
            if mutation == "skip_rescale" and not skipped and t >= 2 * KT and bool(grew.any()):
                skipped = True  # this tile: O keeps the old scale where the row max grew
            else:
                acc = acc * alpha[..., None]
            acc = acc + torch.einsum("brqk,bkd->brqd", _rt(p, dtype), vh[:, t:t + KT])
            m = m_new
        o[:, :, hs] = _rt(acc / l[..., None], dtype).permute(0, 2, 1, 3)
        lse[:, hs] = m + torch.log(l)
    if mutation == "lse_shift":
        lse = lse + 0.02
    o_in, lse_in = (o, lse) if o_lse is None else (o_lse[0].float(), o_lse[1].float())
    if o_lse is not None and mutation == "lse_shift":
        lse_in = lse_in + 0.02
    dq = torch.empty(B, S, Hq, D)
    dk = torch.empty(B, S, Hkv, D)
    dv = torch.empty(B, S, Hkv, D)
    for hs, h in groups:
        qg, kh, vh = q[:, :, hs].float(), k[:, :, h].float(), v[:, :, h].float()
        dog = do[:, :, hs].float()
        if k_prescale:
            s2 = _scores(qg, _rt(kh * (scale * LOG2E), dtype), 1.0, vis)
            p = torch.exp2(s2 - (lse_in[:, hs] * LOG2E)[..., None])
        else:
            p = torch.exp(_scores(qg, kh, scale, vis) - lse_in[:, hs][..., None])
        dp = torch.einsum("bqrd,bkd->brqk", dog, vh)
        delta = (dog * o_in[:, :, hs]).sum(-1).permute(0, 2, 1)
        if mutation == "delta_zero_tail":
            delta = delta.clone()
            delta[..., S - 32:] = 0
        ds = _rt(p * (dp - delta[..., None]), dtype)
        dq[:, :, hs] = (1.0 if mutation == "dq_no_scale" else scale) * torch.einsum("brqk,bkd->bqrd", ds, kh)
        dk[:, :, h] = (scale * scale if mutation == "dk_scale_twice" else scale) * torch.einsum("brqk,bqrd->bkd", ds, qg)
        dv[:, :, h] = torch.einsum("brqk,bqrd->bkd", _rt(p, dtype), dog)
    if mutation == "last_key_zero":
        dk[:, S - 1] = 0
        dv[:, S - 1] = 0
    if rope_tab is not None:
        dq = rope_inverse64(dq.double(), rope_tab, doc_start).float()
        dk = rope_inverse64(dk.double(), rope_tab, doc_start).float()
    return o, lse, _rt(dq, dtype), _rt(dk, dtype), _rt(dv, dtype)


# ------------------------------------------------------------------------------------------------
# input recipes: (q, k, v, do, scale), storage-dtype CPU tensors; the same draws for every dtype
def _seed(name, B, S, Hq, Hkv, D):
    return (RECIPES.index(name) + 1) * 1000003 + B * 7919 + S * 31 + Hq * 17 + Hkv * 5 + D


def recipe(name, B, S, Hq, Hkv, D, dtype, causal=True):
    g = torch.Generator().manual_seed(_seed(name, B, S, Hq, Hkv, D))
    q = torch.randn(B, S, Hq, D, generator=g)
    k = torch.randn(B, S, Hkv, D, generator=g)
    v = torch.randn(B, S, Hkv, D, generator=g)
    do = torch.randn(B, S, Hq, D, generator=g)
    scale = 1.0 / math.sqrt(D)
    if name == "flat":
        pass
    elif name in ("peaked", "peaked_rsqrt"):
        q, k, v, do = 2 * q, 2 * k, v + 1.0, do + 0.5
        scale = 0.25 if name == "peaked" else scale
    elif name in ("stair5", "stair9"):
        # column 0 carries score = c ln2 (key // 64) for every query; the other columns are small noise
        c = float(name[5:])
        q, k, v = 0.25 * q, 0.25 * k, v + 0.5
        q[..., 0] = 4.0
        step = c * math.log(2.0) / (4.0 * scale)
        k[..., 0] = (step * (torch.arange(S) // KT).float()).view(1, S, 1)
    elif name in ("all_negative", "all_large"):
        # column 0 carries -+140 nats; the N(0, 1) rest adds a score of unit variance
        q[..., 0] = 8.0
        k[..., 0] = (-1.0 if name == "all_negative" else 1.0) * 140.0 / (8.0 * scale)
        v, do = v + 0.5, do + 0.25
    elif name == "spike_rows":
        # one query row per 32-row tile points at one key (score ~ 20 nats): the first, a middle and
        # the last key tile in turn, and the causal diagonal (the row's own key)
        rep = Hq // Hkv
        for t in range(S // 32 + (1 if S % 32 else 0)):
            r = min(32 * t + (7 * t) % 32, S - 1)
            j = (3, S // 2 + 5, S - 2, r)[t % 4]
            if causal:
                j = min(j, r)
            q[:, r] = (20.0 / (D * scale)) * k[:, j].repeat_interleave(rep, dim=1)
        v, do = v + 0.5, do + 0.25
    elif name == "odd_scale":
        q, k, scale = q * D ** -0.25, k * D ** -0.25, 1.0
    else:
        raise KeyError(name)
    return q.to(dtype), k.to(dtype), v.to(dtype), do.to(dtype), scale


def doc_starts(B, S):
    """int32 [B, S] for the packed cases: sequence 0 has boundaries inside a 64-key tile (37), on a tile
    edge (128) and three one-token documents (200, 201, 202); the others are one document with a late
    boundary one token before the end."""
    ds = torch.zeros(B, S, dtype=torch.int32)
    for start in (37, 128, 200, 201, 202, 203):
        if start < S:
            ds[0, start:] = start
    if B > 1:
        ds[1:, S - 1] = S - 1
    return ds


def rope_tab(D, S):
    from pyrecover_amd.ops import reference as R

    return R.rope_table(R.precompute_freqs_cis(D, S, 10000.0)).float()


# ------------------------------------------------------------------------------------------------
# a case = inputs + oracle + error scales, computed once on the CPU and shared by the tests
class Case:
    pass


@functools.lru_cache(maxsize=None)
def make_case(name, shape, dtype, causal, packed=False):
    """Inputs (storage dtype), the fp64 oracle and the error scales. The backward oracle runs on the
    oracle's own o rounded to the storage dtype (o_in) and its lse as fp32 (lse_in): what a correct
    forward kernel hands to the backward kernels. dq_rope / dk_rope carry the inverse RoPE."""
    B, S, Hq, Hkv, D = shape
    c = Case()
    c.name, c.shape, c.dtype, c.causal = name, shape, dtype, causal or packed
    c.q, c.k, c.v, c.do, c.scale = recipe(name, B, S, Hq, Hkv, D, dtype, causal or packed)
    c.doc_start = doc_starts(B, S) if packed else None
    c.vis = visibility(B, S, S, c.causal, c.doc_start)
    c.tab = rope_tab(D, S)
    c.o, c.lse = forward_oracle(c.q, c.k, c.v, c.scale, c.vis)
    c.o_in, c.lse_in = c.o.to(dtype), c.lse.float()
    c.dq, c.dk, c.dv = backward_oracle(c.q, c.k, c.v, c.o_in, c.lse_in, c.do, c.scale, c.vis)
    c.dq_rope = rope_inverse64(c.dq, c.tab, c.doc_start)
    c.dk_rope = rope_inverse64(c.dk, c.tab, c.doc_start)
    c.m_o, c.m_dq, c.m_dk, c.m_dv = abs_oracle(c.q, c.k, c.v, c.o_in, c.lse_in, c.do, c.scale, c.vis, dtype)
    c.lse_bound, c.smax = lse_bound(c.q, c.k, c.scale, c.vis, c.lse)
    return c
