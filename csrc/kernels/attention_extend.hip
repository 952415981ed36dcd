// Multi-token KV-cache append ("extend") attention for gfx950, bf16 or fp16, head_dim 64/128, native GQA.
//
// nt new queries per sequence over a cache [B][cap][Hkv][D] that already holds keys. kv_len (int32 [B] on the
// device, clamped into [0, cap] here) is the number of tokens in the cache BEFORE this append; the new
// tokens' own rotated k and plain v are in the cache already (rope_append with nt tokens runs first), so
// the cache is the single source of K and V. Query t of sequence b sits at position p = kv_len[b] + t and
// attends to keys 0 .. min(p, cap - 1): every row sees at least key 0. No launch argument depends on a
// host copy of kv_len.
//
// The structure is the plain forward of attention_docs.hip: 4 waves x 32 rows per block, 64-key K/V
// tiles register-staged into a double LDS buffer, S^T = K Q^T with one query row per lane, the exact
// deferred rescale, a finite "no score yet" running max, the row-per-lane epilogue. Two differences:
//  * Rows are (token, head-of-group) pairs. A block belongs to (row tile, kv head, sequence); its 128
//    rows are r = t * G + g with G = Hq / Hkv, so one pass over K and V serves the whole GQA group and
//    a short append still fills MFMA tiles (8 tokens at G = 4 are one wave). Rows r >= nt * G are
//    clamped for loads and never stored; a wave with no real row skips every tile.
//  * The key bounds come from device memory. A block walks tiles 0 .. bend / 64 with bend the bound of
//    its last query; a wave skips tiles wholly after its own rows' bound; rows are masked only on
//    tiles that cross a row's bound. The staging load's row bound is bend + 1, so no key at or beyond
//    min(kv_len[b] + nt, cap) is ever loaded (zeros stand in, and they are masked): whatever the cache
//    holds there, NaN and Inf included, cannot reach an output.
// One block walks all keys of its rows (no key split), no atomics, one fixed summation order: the same
// bits from run to run, and a sequence's output does not depend on cap or on the rest of the batch.
// Compiled with -fno-honor-nans like attention_docs.hip: no NaN is formed.
#include "attn_common.h"
#include "common.h"
#include "attn_launch.h"

namespace pra {
namespace attn {

constexpr float kNoMax = -1e30f;  // "no score yet" running max (log2 units; real scores are far above)

// grid row tiles x Hkv x B, the row tile slowest and descending. Q rows are [B * nt][ldq] (a view of the fused QKV activation), O is
// [B][nt][Hq][D] contiguous, LSE fp32 [B][nt][Hq].
template <typename T, int D>
__global__ __launch_bounds__(256, 2) void extend_fwd_kernel(const T* __restrict__ Q, const T* __restrict__ K,
                                                            const T* __restrict__ V, T* __restrict__ O,
                                                            float* __restrict__ LSE, const int* __restrict__ KVLEN,
                                                            int nt, int Hq, int Hkv, int cap, long ldq,
                                                            float scale_log2) {
  constexpr int NW = 4, KT = 64, QT = 32 * NW;
  constexpr int NKS = D / 16, NDB = D / 32, TILE = KT * D;
  __shared__ __attribute__((aligned(16))) T smem[4 * TILE];  // K0 V0 K1 V1

  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, h2 = lane >> 5, l32 = lane & 31;
  const int G = Hq / Hkv, R = nt * G;  // rows of a (sequence, kv head)
  const int nrt = (R + QT - 1) / QT;
  const int BH = gridDim.x / nrt;
  const int rt = nrt - 1 - (int)(blockIdx.x / BH);  // late row tiles first: they walk the most keys
  const int bh = blockIdx.x % BH;
  const int hk = bh % Hkv, b = bh / Hkv;
  const int r0 = rt * QT, rw = r0 + wid * 32;
  const int row = rw + l32;
  const int rc = min(row, R - 1);  // rows past the end repeat the last one and are not stored
  const int t = rc / G, hq = hk * G + rc % G;

  const int len = min(max(KVLEN[b], 0), cap);
  const int kend = min(len + t, cap - 1);                              // this row's last visible key
  const int bend = min(len + min(r0 + QT - 1, R - 1) / G, cap - 1);    // the block's
  const bool active = rw < R;                                          // wave-uniform: the wave has a real row
  const int wlo = min(len + min(rw, R - 1) / G, cap - 1);              // the wave's smallest bound
  const int whi = active ? min(len + min(rw + 31, R - 1) / G, cap - 1) : -1;  // and its largest

  const long ldkv = (long)Hkv * D;
  const T* Kb = K + (long)b * cap * ldkv + hk * D;
  const T* Vb = V + (long)b * cap * ldkv + hk * D;
  const T* Qr = Q + ((long)b * nt + t) * ldq + hq * D + 8 * h2;

  LaneOff<T, D> lo;
  lo.init(lane);
  V8<T> qf[NKS];
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) qf[ks] = *reinterpret_cast<const V8<T>*>(Qr + 16 * ks);

  f32x16 o[NDB];
#pragma unroll
  for (int i = 0; i < NDB; ++i) o[i] = f32x16{};
  float m_i = kNoMax, l_i = 0.f;

  const int nkt = bend / KT + 1;  // bend >= 0: at least one tile
  const int nvalid = bend + 1;    // rows of the cache the block may load (<= min(len + nt, cap))

  Stage<T, D, KT, NW * 64> sk, sv;
  sk.load(Kb, ldkv, 0, nvalid);
  sv.load(Vb, ldkv, 0, nvalid);
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
      sk.load(Kb, ldkv, k0 + KT, nvalid);
      sv.load(Vb, ldkv, k0 + KT, nvalid);
    }
    if (k0 <= whi) {  // wave-uniform: else the tile lies wholly after the wave's rows' bounds
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
      if (k0 + KT - 1 > wlo) {  // the tile crosses some row's bound
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int ka = k0 + crow(r, h2), kb = ka + 32;
          if (ka > kend) s0[r] = -INFINITY;
          if (kb > kend) s1[r] = -INFINITY;
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
  for (int kt = 0; kt < nkt; kt += 2) {
    body(IC<0>{}, kt);
    if (kt + 1 < nkt) body(IC<1>{}, kt + 1);
  }

  // a real row saw key 0 at least: l_i > 0. A wave without real rows kept l_i = 0 and stores nothing.
  const bool ok = row < R;
  const float inv = l_i > 0.f ? 1.f / l_i : 0.f;
  const long orow = ((long)b * nt + t) * Hq + hq;
  store_rows16<T, NDB>(o, inv, O + orow * D, ok, h2);  // all 64 lanes: the lane swap
  if (ok && h2 == 0) LSE[orow] = (m_i + __log2f(l_i)) * 0.69314718055994531f;
}

}  // namespace attn
}  // namespace pra

extern "C" hipError_t pra_attn_extend(int dtype, const void* q, long ldq, const void* k_cache, const void* v_cache,
                                      const int* kv_len, void* o, float* lse, int B, int T, int Hq, int Hkv, int D,
                                      int cap, float scale, hipStream_t s) {
  using namespace pra::attn;
  if (q == nullptr || k_cache == nullptr || v_cache == nullptr || kv_len == nullptr || o == nullptr || lse == nullptr)
    return hipErrorInvalidValue;
  if (B <= 0 || T <= 0 || cap <= 0 || Hq <= 0 || Hkv <= 0 || Hq % Hkv || (D != 64 && D != 128) || ldq % 8 ||
      ldq < (long)Hq * D || (long)T * (Hq / Hkv) > 0x7fffffffL - 128 || (long)cap > 0x7fffffffL / 2)
    return hipErrorInvalidValue;
  const int R = T * (Hq / Hkv);
  const long blocks = (long)((R + 127) / 128) * Hkv * B;
  if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
  const dim3 grid((unsigned)blocks), block(256);
  const float sl2 = scale * kLog2e;
  return dispatch_16bit(dtype, [&](auto t) {
    using E = decltype(t);
    pra::dispatch(
        [&](auto d) {
          hipLaunchKernelGGL((extend_fwd_kernel<E, d()>), grid, block, 0, s, (const E*)q, (const E*)k_cache,
                             (const E*)v_cache, (E*)o, lse, kv_len, T, Hq, Hkv, cap, ldq, sl2);
        },
        HeadDim{D});
    return hipGetLastError();
  });
}
