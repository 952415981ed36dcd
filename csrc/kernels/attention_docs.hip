// Document-masked ("packed sequence") causal flash attention for gfx950, bf16 or fp16, head_dim
// 64/128, native GQA. A row of S tokens holds several documents back to back; doc_start[b][i] is the
// index within row b of the first token of token i's document, and query i sees key j iff
// doc_start[b][i] <= j <= i. Every value read from doc_start is clamped into [0, i], so whatever the
// tensor holds, the mask leaves row i at least its own key and no access leaves the row.
//
// Three kernels in the structure of the plain (non-pipelined) kernels of attention.hip, all with
// 4 waves x 32 rows = 128-row blocks (the finest block the tile skipping can work with):
//  * forward (fwd_kernel): the key loop starts at the 64-key tile that holds the smallest
//    doc_start of the block's 128 query rows; a wave skips tiles before its own 32 rows' smallest.
//  * dQ (bwd_dq_kernel<PIPE = false>): the same key-loop start; also publishes delta.
//  * dK/dV (bwd_dkdv_kernel, NW = 4): the query loop ends at the last query whose document reaches
//    into the block's 128 keys; that bound comes from a pre-pass kernel (one block per key block,
//    no host synchronisation, capturable).
// So a row of n equal documents costs about 1/n of the causal S^2 / 2, at 128-row granularity.
// No atomics and a fixed summation order: results are bit-reproducible from run to run.
//
// Fully masked rows inside a processed tile (a document boundary inside a wave's 32 rows): the
// forward's running max starts at a large negative finite value instead of -inf, so a row whose
// scores so far are all -inf computes exp2(-inf + 1e30) = 0 and never forms -inf + inf (the file is
// compiled with -fno-honor-nans: no NaN may be produced, and none is tested for). The backward
// masks p with a select.
#include "attn_common.h"
#include "common.h"
#include "attn_launch.h"

namespace pra {
namespace attn {

constexpr float kNoMax = -1e30f;  // "no score yet" running max (log2 units; real scores are far above)

__device__ __forceinline__ int doc_clamp(int ds, int i) { return min(max(ds, 0), i); }
__device__ __forceinline__ int wave_min(int x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x = min(x, __shfl_xor(x, off));
  return x;
}
__device__ __forceinline__ int wave_max(int x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x = max(x, __shfl_xor(x, off));
  return x;
}

// ======================================================================================
// Forward: block = (b, q head, 128 query rows); 64-key K/V tiles register-staged into a double
// buffer, "swapped" products (one query per lane), exact deferred rescale (see fwd_kernel).
// S % 128 == 0.
// ======================================================================================
template <typename T, int D>
__global__ __launch_bounds__(256, 2) void docs_fwd_kernel(const T* __restrict__ Q, const T* __restrict__ K,
                                                          const T* __restrict__ V, T* __restrict__ O,
                                                          float* __restrict__ LSE, const int* __restrict__ DS, int S,
                                                          int Hq, int Hkv, long ldq, long ldk, long ldv, long ldo,
                                                          float scale_log2) {
  constexpr int NW = 4, KT = 64, QT = 32 * NW;
  constexpr int NKS = D / 16, NDB = D / 32, TILE = KT * D;
  __shared__ __attribute__((aligned(16))) T smem[4 * TILE];  // K0 V0 K1 V1
  __shared__ int wmin_s[NW];

  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, h2 = lane >> 5, l32 = lane & 31;
  const int nqt = S / QT;
  const int BH = gridDim.x / nqt;
  const int qt = nqt - 1 - (int)(blockIdx.x / BH);  // late query tiles first
  const int bh = blockIdx.x % BH;
  const int hq = bh % Hq, b = bh / Hq;
  const int hk = hq / (Hq / Hkv);
  const int q0 = qt * QT, qw = q0 + wid * 32;
  const int qrow = qw + l32;  // < S

  const T* Qb = Q + (long)b * S * ldq + hq * D;
  const T* Kb = K + (long)b * S * ldk + hk * D;
  const T* Vb = V + (long)b * S * ldv + hk * D;

  const int ds = doc_clamp(DS[(long)b * S + qrow], qrow);
  const int wmin = wave_min(ds), wmax = wave_max(ds);
  if (lane == 0) wmin_s[wid] = wmin;

  LaneOff<T, D> lo;
  lo.init(lane);
  V8<T> qf[NKS];
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) qf[ks] = *reinterpret_cast<const V8<T>*>(Qb + (long)qrow * ldq + 16 * ks + 8 * h2);

  f32x16 o[NDB];
#pragma unroll
  for (int i = 0; i < NDB; ++i) o[i] = f32x16{};
  float m_i = kNoMax, l_i = 0.f;

  __syncthreads();
  const int bmin = min(min(wmin_s[0], wmin_s[1]), min(wmin_s[2], wmin_s[3]));
  const int kt0 = bmin / KT;            // first key tile any row of the block can see
  const int nkt = (q0 + QT) / KT;       // causal end (q0 + QT <= S)

  Stage<T, D, KT, NW * 64> sk, sv;
  sk.load(Kb, ldk, kt0 * KT, S);
  sv.load(Vb, ldv, kt0 * KT, S);
  sk.store(smem);
  sv.store(smem + TILE);
  __syncthreads();

  auto body = [&](auto cc, int kt) {
    constexpr int CUR = decltype(cc)::value;
    const T* Kt = smem + 2 * CUR * TILE;
    const T* Vt = Kt + TILE;
    const int k0 = kt * KT;
    const bool more = kt + 1 < nkt;
    if (more) {
      sk.load(Kb, ldk, k0 + KT, S);
      sv.load(Vb, ldv, k0 + KT, S);
    }
    // wave-uniform: the tile lies wholly after the wave's queries or before their documents
    if (!(k0 > qw + 31 || k0 + KT - 1 < wmin)) {
      f32x16 s0 = f32x16{}, s1 = f32x16{};
      V8<T> a0 = lo.rowk(Kt, 0, 0), a1 = lo.rowk(Kt, 32, 0);
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) {
        V8<T> n0 = a0, n1 = a1;
        if (ks + 1 < NKS) {
          n0 = lo.rowk(Kt, 0, ks + 1);
          n1 = lo.rowk(Kt, 32, ks + 1);
        }
        s0 = mfma(a0, qf[ks], s0);
        s1 = mfma(a1, qf[ks], s1);
        a0 = n0;
        a1 = n1;
      }
      if (k0 + KT - 1 > qw || k0 < wmax) {  // diagonal tile or a document boundary inside it
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int ka = k0 + crow(r, h2), kb = ka + 32;
          if (ka > qrow || ka < ds) s0[r] = -INFINITY;
          if (kb > qrow || kb < ds) s1[r] = -INFINITY;
        }
      }
      float mx = -INFINITY;
#pragma unroll
      for (int r = 0; r < 16; ++r) mx = fmaxf(mx, fmaxf(s0[r], s1[r]));
      mx = half_max(mx) * scale_log2;  // -inf for a row with no visible key in this tile
      if (!__all(mx <= m_i)) {
        const float m_new = fmaxf(m_i, mx);  // finite: m_i is
        const float alpha = fexp2(m_i - m_new);
        l_i *= alpha;
#pragma unroll
        for (int i = 0; i < NDB; ++i) o[i] *= alpha;
        m_i = m_new;
      }
      float rs = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        s0[r] = fexp2(fmaf(s0[r], scale_log2, -m_i));  // masked: exp2(-inf) = 0, m_i finite
        s1[r] = fexp2(fmaf(s1[r], scale_log2, -m_i));
        rs += s0[r] + s1[r];
      }
      l_i += half_sum(rs);
      const V8<T> p00 = pack8<T>(s0, 0), p01 = pack8<T>(s0, 1), p10 = pack8<T>(s1, 0), p11 = pack8<T>(s1, 1);
      V8<T> vc = lo.tr(Vt, 0, 0);
#pragma unroll
      for (int st = 0; st < 4 * NDB; ++st) {
        const int k4 = st / NDB, db = st % NDB;
        V8<T> vn = vc;
        if (st + 1 < 4 * NDB) vn = lo.tr(Vt, ((st + 1) / NDB) * 16, (st + 1) % NDB);
        const V8<T> pf = k4 == 0 ? p00 : k4 == 1 ? p01 : k4 == 2 ? p10 : p11;
        o[db] = mfma(vc, pf, o[db]);
        vc = vn;
      }
    }
    if (more) {
      sk.store(smem + 2 * (1 - CUR) * TILE);
      sv.store(smem + 2 * (1 - CUR) * TILE + TILE);
    }
    __syncthreads();
  };
  for (int kt = kt0; kt < nkt; kt += 2) {
    body(IC<0>{}, kt);
    if (kt + 1 < nkt) body(IC<1>{}, kt + 1);
  }

  const float inv = 1.f / l_i;  // l_i > 0: every row sees its own key
  store_rows16<T, NDB>(o, inv, O + ((long)b * S + qrow) * ldo + hq * D, true, h2);
  if (h2 == 0) LSE[((long)b * Hq + hq) * S + qrow] = (m_i + __log2f(l_i)) * 0.69314718055994531f;
}

// ======================================================================================
// Backward dQ: block = (b, q head, 128 query rows); 64-key K/V tiles by LDS-DMA into a double
// buffer (see bwd_dq_kernel). Publishes delta = rowsum(dO * O) for the dK/dV kernel.
// rtab: inverse RoPE on dQ with the packed position qrow - doc_start.
// ======================================================================================
template <typename T, int D>
__global__ __launch_bounds__(256, 2) void docs_bwd_dq_kernel(
    const T* __restrict__ Q, const T* __restrict__ K, const T* __restrict__ V, const T* __restrict__ dO,
    const T* __restrict__ O, const float* __restrict__ LSE, float* __restrict__ Delta, T* __restrict__ dQ,
    const int* __restrict__ DS, int S, int Hq, int Hkv, long ldq, long ldk, long ldv, long lddo, long ldo, long lddq,
    float scale, float scale_log2, int skv, const float2* __restrict__ rtab) {
  constexpr int NW = 4, KT = 64, QT = 32 * NW;
  constexpr int NKS = D / 16, NDB = D / 32, TILE = KT * D;
  __shared__ __attribute__((aligned(16))) T kvb0[2 * TILE];
  __shared__ __attribute__((aligned(16))) T kvb1[2 * TILE];
  __shared__ int wmin_s[NW];

  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, h2 = lane >> 5, l32 = lane & 31;
  const int nqt = S / QT;
  const int BH = gridDim.x / nqt;
  const int qt = nqt - 1 - (int)(blockIdx.x / BH);
  const int bh = blockIdx.x % BH;
  const int hq = bh % Hq, b = bh / Hq;
  const int hk = hq / (Hq / Hkv);
  const int q0 = qt * QT, qw = q0 + wid * 32;
  const int qrow = qw + l32;  // < S

  const T* Kb = K + (long)b * S * ldk + hk * D;
  const T* Vb = V + (long)b * S * ldv + hk * D;

  const int ds = doc_clamp(DS[(long)b * S + qrow], qrow);
  const int wmin = wave_min(ds);
  if (lane == 0) wmin_s[wid] = wmin;

  LaneOff<T, D> lo;
  lo.init(lane);
  V8<T> qf[NKS], df[NKS];
  {
    const T* Qr = Q + ((long)b * S + qrow) * ldq + hq * D + 8 * h2;
    const T* Dr = dO + ((long)b * S + qrow) * lddo + hq * D + 8 * h2;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      qf[ks] = *reinterpret_cast<const V8<T>*>(Qr + 16 * ks);
      df[ks] = *reinterpret_cast<const V8<T>*>(Dr + 16 * ks);
    }
  }
  float lse2, dl;
  {
    float part = 0.f;
    const long i = ((long)b * Hq + hq) * S + qrow;
    lse2 = LSE[i] * kLog2e;
    const T* Orow = O + ((long)b * S + qrow) * ldo + hq * D + 8 * h2;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      const V8<T> o8 = *reinterpret_cast<const V8<T>*>(Orow + 16 * ks);
#pragma unroll
      for (int j = 0; j < 8; ++j) part = fmaf((float)o8[j], (float)df[ks][j], part);
    }
    dl = half_sum(part);
    if (h2 == 0) Delta[i] = dl;
  }

  f32x16 dqt[NDB];
#pragma unroll
  for (int i = 0; i < NDB; ++i) dqt[i] = f32x16{};

  __syncthreads();
  const int bmin = min(min(wmin_s[0], wmin_s[1]), min(wmin_s[2], wmin_s[3]));
  const int kt0 = bmin / KT;
  const int nkt = (q0 + QT) / KT;

  GStage<T, D, KT, NW> gk, gv;
  gk.init(ldk);
  gv.init(ldv);
  gk.issue(Kb + (long)kt0 * KT * ldk, kvb0);
  gv.issue(Vb + (long)kt0 * KT * ldv, kvb0 + TILE);
  __syncthreads();
  auto body = [&](auto cc, int kt) {
    constexpr int CUR = decltype(cc)::value;
    T* const cur_b = CUR ? kvb1 : kvb0;
    T* const oth_b = CUR ? kvb0 : kvb1;
    const T* Kt = cur_b;
    const T* Vt = Kt + TILE;
    const int k0 = kt * KT;
    if (kt + 1 < nkt) {  // k0 + 2 KT <= q0 + QT <= S: the next tile is in the row
      gk.issue(Kb + (long)(k0 + KT) * ldk, oth_b);
      gv.issue(Vb + (long)(k0 + KT) * ldv, oth_b + TILE);
    }
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      const int kh = k0 + 32 * kb;
      if (kh > qw + 31 || kh + 31 < wmin) continue;  // wave-uniform: this key half is fully masked
      f32x16 s = f32x16{}, dp = f32x16{};
      V8<T> ka = lo.rowk(Kt, 32 * kb, 0), va = lo.rowk(Vt, 32 * kb, 0);
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) {
        V8<T> nk = ka, nv = va;
        if (ks + 1 < NKS) {
          nk = lo.rowk(Kt, 32 * kb, ks + 1);
          nv = lo.rowk(Vt, 32 * kb, ks + 1);
        }
        s = mfma(ka, qf[ks], s);
        dp = mfma(va, df[ks], dp);
        ka = nk; va = nv;
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = kh + crow(r, h2);
        float p = fexp2(fmaf(s[r], scale_log2, -lse2));
        if (key > qrow || key < ds) p = 0.f;
        dp[r] = p * (dp[r] - dl);
      }
      const V8<T> d0 = pack8<T>(dp, 0), d1 = pack8<T>(dp, 1);
      V8<T> kc = lo.tr(Kt, 32 * kb, 0);
#pragma unroll
      for (int st = 0; st < 2 * NDB; ++st) {
        const int s2 = st / NDB, db = st % NDB;
        V8<T> kn = kc;
        if (st + 1 < 2 * NDB) kn = lo.tr(Kt, 32 * kb + 16 * ((st + 1) / NDB), (st + 1) % NDB);
        dqt[db] = mfma(kc, s2 ? d1 : d0, dqt[db]);
        kc = kn;
      }
    }
    __syncthreads();
  };
  for (int kt = kt0; kt < nkt; kt += 2) {
    body(IC<0>{}, kt);
    if (kt + 1 < nkt) body(IC<1>{}, kt + 1);
  }

  // packed RoPE position of the row (zero-padded rows >= skv are discarded: clamp them into the table)
  store_rows16<T, NDB>(dqt, scale, dQ + ((long)b * S + qrow) * lddq + hq * D, true, h2,
                       rtab ? rtab + (long)max(min(qrow, skv - 1) - ds, 0) * (D / 2) : nullptr);
}

// ======================================================================================
// Pre-pass of the dK/dV kernel: QEND[b][kb] = end (exclusive, a multiple of 32) of the query rows
// that see any of the key block's 128 keys = 1 + the last i with doc_start[b][i] <= k0 + 127. A
// full scan, so the bound is exact for any doc_start (for a non-decreasing one a search would do).
// ======================================================================================
__global__ __launch_bounds__(256) void docs_qend_kernel(const int* __restrict__ DS, int* __restrict__ QEND, int S) {
  constexpr int KB = 128;
  __shared__ int wm[4];
  const int nkb = S / KB, kb = blockIdx.x % nkb, b = blockIdx.x / nkb;
  const int klast = kb * KB + KB - 1;
  const int* row = DS + (long)b * S;
  int last = klast;  // the block's own rows always reach it
  for (int i = kb * KB + threadIdx.x; i < S; i += 256)
    if (doc_clamp(row[i], i) <= klast) last = max(last, i);
  last = wave_max(last);
  if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = last;
  __syncthreads();
  if (threadIdx.x == 0) QEND[blockIdx.x] = (max(max(wm[0], wm[1]), max(wm[2], wm[3])) / 32 + 1) * 32;
}

// ======================================================================================
// Backward dK/dV: block = (b, kv head, 128 keys), K/V resident in LDS, 32-row Q/dO tiles streamed
// through one LDS buffer (see bwd_dkdv_kernel, NW = 4). The query loop runs over [k0, QEND). The
// tiles fill 80 KB of LDS exactly (two blocks per CU at D = 128), so the tile's per-row values
// (lse, delta, doc_start) live one row per lane and are broadcast with ds_bpermute.
// ======================================================================================
template <typename T, int D>
__global__ __launch_bounds__(256, 2) void docs_bwd_dkdv_kernel(
    const T* __restrict__ Q, const T* __restrict__ K, const T* __restrict__ V, const T* __restrict__ dO,
    const float* __restrict__ LSE, const float* __restrict__ Delta, T* __restrict__ dK, T* __restrict__ dV,
    const int* __restrict__ DS, const int* __restrict__ QEND, int S, int Hq, int Hkv, long ldq, long ldk, long ldv,
    long lddo, long lddk, long lddv, float scale, float scale_log2, int skv, const float2* __restrict__ rtab) {
  constexpr int NW = 4, KB = 32 * NW, QT = 32, NT = NW * 64;
  constexpr int NKS = D / 16, NDB = D / 32;
  constexpr int KVT = KB * D, QDT = QT * D;
  __shared__ __attribute__((aligned(16))) T smem[2 * KVT + 2 * QDT];  // Q dO K V
  T* const Qs = smem;
  T* const Ds = smem + QDT;
  T* const Ks = smem + 2 * QDT;
  T* const Vs = smem + 2 * QDT + KVT;

  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, h2 = lane >> 5, l32 = lane & 31;
  const int nkb = S / KB;
  const int BH = gridDim.x / nkb;
  const int kbk = blockIdx.x / BH;  // early key blocks first
  const int bh = blockIdx.x % BH;
  const int hk = bh % Hkv, b = bh / Hkv;
  const int nrep = Hq / Hkv;
  const int k0 = kbk * KB, kw = k0 + wid * 32;
  const int krow = kw + l32;  // < S

  {
    GStage<T, D, KB, NW> gk, gv;
    gk.init(ldk);
    gv.init(ldv);
    gk.issue(K + ((long)b * S + k0) * ldk + hk * D, Ks);
    gv.issue(V + ((long)b * S + k0) * ldv + hk * D, Vs);
  }
  const T* Kw = Ks + wid * 32 * D;
  const T* Vw = Vs + wid * 32 * D;
  LaneOff<T, D> lo;
  lo.init(lane);

  f32x16 dkt[NDB], dvt[NDB];
#pragma unroll
  for (int i = 0; i < NDB; ++i) { dkt[i] = f32x16{}; dvt[i] = f32x16{}; }

  const int qstart = k0;
  const int qend = min(max(QEND[b * nkb + kbk], k0 + KB), S);  // in [k0 + 128, S], a multiple of 32
  const int nqt = (qend - qstart) / QT;
  const int total = nqt * nrep;
  const float rc_mul = h2 ? 1.f : kLog2e;
  const float* rc_base = (h2 ? Delta : LSE) + (long)b * Hq * S + l32;
  const int* ds_base = DS + (long)b * S + l32;
  int bp_base = 4 * (4 * h2);  // ds_bpermute byte address of lane crow(0, h2)
  asm volatile("" : "+v"(bp_base));

  Stage<T, D, QT, NT> sq, sd;
  auto stage_load = [&](int it) {
    const int hq = hk * nrep + it / nqt;
    const int q0 = qstart + (it % nqt) * QT;
    sq.load(Q + (long)b * S * ldq + hq * D, ldq, q0, S);
    sd.load(dO + (long)b * S * lddo + hq * D, lddo, q0, S);
  };
  stage_load(0);

  for (int it = 0; it < total; ++it) {
    const int hq = hk * nrep + it / nqt;
    const int q0 = qstart + (it % nqt) * QT;
    sq.store(Qs);
    sd.store(Ds);
    const float rcv = rc_base[(long)hq * S + q0] * rc_mul;
    const int dsv = doc_clamp(ds_base[q0], q0 + l32);  // row l32 of the tile (q0 + l32 < qend <= S)
    const int dmin = wave_min(dsv);
    __syncthreads();
    if (it + 1 < total) stage_load(it + 1);
    // wave-uniform: the tile lies wholly before the wave's keys, or its documents start after them
    if (!(q0 + QT - 1 < kw || dmin > kw + 31)) {
      f32x16 s = f32x16{}, dp = f32x16{};
      V8<T> xa = lo.rowk(Qs, 0, 0), xb = lo.rowk(Kw, 0, 0);
#pragma unroll
      for (int st = 0; st < 2 * NKS; ++st) {
        V8<T> na = xa, nb = xb;
        if (st + 1 < 2 * NKS) {
          const int nks = (st + 1) % NKS;
          na = lo.rowk(st + 1 < NKS ? Qs : Ds, 0, nks);
          nb = lo.rowk(st + 1 < NKS ? Kw : Vw, 0, nks);
        }
        if (st < NKS) s = mfma(xa, xb, s);
        else dp = mfma(xa, xb, dp);
        xa = na; xb = nb;
      }
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        float lse4[4], dl4[4];
        int dsr[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int src = bp_base + 4 * (j + 8 * rr);  // lane crow(4 rr + j, h2)
          lse4[j] = __int_as_float(__builtin_amdgcn_ds_bpermute(src, __float_as_int(rcv)));
          dl4[j] = __int_as_float(__builtin_amdgcn_ds_bpermute(src + 128, __float_as_int(rcv)));
          dsr[j] = __builtin_amdgcn_ds_bpermute(src, dsv);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int r = 4 * rr + j;
          float p = fexp2(fmaf(s[r], scale_log2, -lse4[j]));
          if (krow > q0 + crow(r, h2) || krow < dsr[j]) p = 0.f;
          s[r] = p;
          dp[r] = p * (dp[r] - dl4[j]);
        }
      }
      const V8<T> p0 = pack8<T>(s, 0), p1 = pack8<T>(s, 1), d0 = pack8<T>(dp, 0), d1 = pack8<T>(dp, 1);
      V8<T> ot = lo.tr(Ds, 0, 0), qt = lo.tr(Qs, 0, 0);
#pragma unroll
      for (int st = 0; st < 2 * NDB; ++st) {
        const int s2 = st / NDB, db = st % NDB;
        V8<T> no = ot, nq = qt;
        if (st + 1 < 2 * NDB) {
          no = lo.tr(Ds, 16 * ((st + 1) / NDB), (st + 1) % NDB);
          nq = lo.tr(Qs, 16 * ((st + 1) / NDB), (st + 1) % NDB);
        }
        dvt[db] = mfma(ot, s2 ? p1 : p0, dvt[db]);
        dkt[db] = mfma(qt, s2 ? d1 : d0, dkt[db]);
        ot = no; qt = nq;
      }
    }
    __syncthreads();
  }

  const int dsk = doc_clamp(DS[(long)b * S + krow], krow);
  store_rows16<T, NDB>(dkt, scale, dK + ((long)b * S + krow) * lddk + hk * D, true, h2,
                       rtab ? rtab + (long)max(min(krow, skv - 1) - dsk, 0) * (D / 2) : nullptr);
  store_rows16<T, NDB>(dvt, 1.f, dV + ((long)b * S + krow) * lddv + hk * D, true, h2);
}

namespace {

// the only family that bounds its grid and rejects B, Hkv <= 0
bool docs_shape_ok(const pra_attn_args& a, bool bwd) {
  return a.B > 0 && a.S > 0 && a.S % 128 == 0 && (a.D == 64 || a.D == 128) && a.Hkv > 0 && a.Hq % a.Hkv == 0 &&
         (long)a.B * a.Hq * (a.S / 128) <= 0x7fffffffL && a.doc_start != nullptr && strides_ok(a, bwd, 8);
}

}  // namespace

hipError_t docs_fwd(const pra_attn_args& a, hipStream_t st) {
  if (!docs_shape_ok(a, false)) return hipErrorInvalidValue;
  const dim3 grid((a.S / 128) * a.Hq * a.B), block(256);
  const float sl2 = a.scale * kLog2e;
  return dispatch_16bit(a.dtype, [&](auto t) {
    using T = decltype(t);
    dispatch(
        [&](auto d) {
          hipLaunchKernelGGL((docs_fwd_kernel<T, d()>), grid, block, 0, st, (const T*)a.q,
                             (const T*)a.k, (const T*)a.v, (T*)a.o, a.lse, a.doc_start, a.S, a.Hq, a.Hkv, a.ldq, a.ldk,
                             a.ldv, a.ldo, sl2);
        },
        HeadDim{a.D});
    return hipGetLastError();
  });
}

hipError_t docs_bwd(const pra_attn_args& a, const BwdPlan& pl, hipStream_t st) {
  if (!docs_shape_ok(a, true) || a.skv <= 0 || a.skv > a.S) return hipErrorInvalidValue;
  const int B = a.B, S = a.S, Hq = a.Hq, Hkv = a.Hkv;
  const float2* rt = reinterpret_cast<const float2*>(a.rope_tab);
  const float scale = a.scale, sl2 = scale * kLog2e;
  const int* ds = a.doc_start;
  float* delta = a.ws + pl.delta;
  int* qend = reinterpret_cast<int*>(a.ws + pl.qend);
  const HeadDim d_{a.D};
  return dispatch_16bit(a.dtype, [&](auto t) {
    using T = decltype(t);
    const T *q = (const T*)a.q, *k = (const T*)a.k, *v = (const T*)a.v, *dout = (const T*)a.dout;
    hipLaunchKernelGGL(docs_qend_kernel, dim3(B * (S / 128)), dim3(256), 0, st, ds, qend, S);
    dispatch(
        [&](auto d) {
          hipLaunchKernelGGL((docs_bwd_dq_kernel<T, d()>), dim3((S / 128) * Hq * B), dim3(256), 0, st,
                             q, k, v, dout, (const T*)a.o, a.lse, delta, (T*)a.dq, ds, S, Hq, Hkv, a.ldq, a.ldk, a.ldv,
                             a.lddo, a.ldo, a.lddq, scale, sl2, a.skv, rt);
        },
        d_);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (a.mid_event != nullptr) {  // the side-stream window opens between dQ and dK/dV
      e = hipEventRecord(a.mid_event, st);
      if (e != hipSuccess) return e;
    }
    dispatch(
        [&](auto d) {
          hipLaunchKernelGGL((docs_bwd_dkdv_kernel<T, d()>), dim3((S / 128) * Hkv * B), dim3(256), 0,
                             st, q, k, v, dout, a.lse, (const float*)delta, (T*)a.dk, (T*)a.dv, ds, (const int*)qend,
                             S, Hq, Hkv, a.ldq, a.ldk, a.ldv, a.lddo, a.lddk, a.lddv, scale, sl2, a.skv, rt);
        },
        d_);
    return hipGetLastError();
  });
}

}  // namespace attn
}  // namespace pra
