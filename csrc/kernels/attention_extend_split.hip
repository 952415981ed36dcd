// Key-split multi-token append attention for gfx950: attention_extend.hip's kernel cut along the keys, for a
// short append (few rows r = t * G + g per kv head) over a long cache, where the single pass leaves one
// wave of one block per (kv head, sequence) walking every key tile while most CUs idle.
//
// Two splits, both with one fixed summation order:
//  * Key chunks. Keys are cut at multiples of kExtendChunk (attn_extend_plan.h): a function of the key
//    position alone, never of cap, kv_len, T or the batch. A block belongs to (row tile, kv head, sequence,
//    chunk c) and walks only the 64-key tiles of [c * XC, min((c + 1) * XC - 1, bend)], bend the bound of
//    its last query; a block whose chunk starts after bend leaves at once and writes nothing. Its fp32
//    partial per row -- unnormalised o[D] and (running max in log2 units, sum) -- goes to a workspace,
//    and extend_combine_kernel merges a row's chunks 0 .. kend / XC in ascending order (as
//    attention_decode.hip does for one query).
//  * Waves. With R <= 32 rows three of the four waves of extend_fwd_kernel have no row. Here the WS waves
//    (4, 2 or 1) that share a 32-row sub-tile hold the same Q fragments and take every WS-th key tile of
//    the chunk, so a block covers 128 / WS rows; all four waves still stage every tile. After the last
//    tile waves 1 .. WS - 1 put their (m, l, o) into the K/V buffers, free by then, and wave 0 folds them
//    in, in wave order (three states of 64 x (D / 2 + 2) floats fit the buffer; wave 0's stays in
//    registers).
// Everything else is extend_fwd_kernel's: S^T = K Q^T with one query row per lane, the exact deferred
// rescale, the finite "no score yet" running max, masking and load bounds from kv_len in device memory
// (no key at or beyond min(kv_len[b] + T, cap) is loaded). No atomics, no workgroup waits for another:
// the same bits from run to run, and a sequence's output does not depend on cap or on the rest of the
// batch. Against the single pass only the order of the fp32 sums differs.
// Compiled with -fno-honor-nans like attention_extend.hip: no NaN is formed.
// The tile loop, the wave fold and the partial store exist three times and are kept in step by hand: here, in
// attention_extend.hip (the single pass) and in attention_extend_fp8.hip (both arms over an fp8 cache).
#include "attn_common.h"
#include "common.h"
#include "attn_launch.h"

namespace pra {
namespace attn {

constexpr float kSplitNoMax = -1e30f;  // attention_extend.hip's kNoMax

// grid (row tiles x Hkv x B) x NC, the chunk fastest, the row tile slowest and descending. Q rows are
// [B * nt][ldq], WO fp32 [B][nt][Hq][NC][D], WML fp32 [B][nt][Hq][NC][2] = (max, sum).
template <typename T, int D, int WS>
__global__ __launch_bounds__(256, 2) void extend_split_kernel(const T* __restrict__ Q, const T* __restrict__ K,
                                                              const T* __restrict__ V, float* __restrict__ WO,
                                                              float* __restrict__ WML, const int* __restrict__ KVLEN,
                                                              int nt, int Hq, int Hkv, int cap, int NC, long ldq,
                                                              float scale_log2) {
  constexpr int NW = 4, KT = 64, NSUB = NW / WS, QT = 32 * NSUB, XC = kExtendChunk;
  constexpr int NKS = D / 16, NDB = D / 32, TILE = KT * D;
  constexpr int NV = 4 * NDB + 1;  // float4 words of one lane's (o, m, l)
  static_assert((NW - NSUB) * NV * 64 * 16 <= 4 * TILE * (int)sizeof(T), "the merged states must fit the tile buffer");
  __shared__ __attribute__((aligned(16))) T smem[4 * TILE];  // K0 V0 K1 V1

  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, h2 = lane >> 5, l32 = lane & 31;
  const int sub = wid / WS, kw = wid % WS;  // the wave's 32-row sub-tile, and its share of the key tiles
  const int G = Hq / Hkv, R = nt * G;
  const int nrt = (R + QT - 1) / QT;
  const int c = blockIdx.x % NC;
  const int rest = blockIdx.x / NC;
  const int BH = gridDim.x / NC / nrt;
  const int rt = nrt - 1 - rest / BH;
  const int bh = rest % BH;
  const int hk = bh % Hkv, b = bh / Hkv;
  const int r0 = rt * QT, rw = r0 + sub * 32;
  const int row = rw + l32;
  const int rc = min(row, R - 1);  // rows past the end repeat the last one and are not stored
  const int t = rc / G, hq = hk * G + rc % G;

  const int len = min(max(KVLEN[b], 0), cap);
  const int kend = min(len + t, cap - 1);                            // this row's last visible key
  const int bend = min(len + min(r0 + QT - 1, R - 1) / G, cap - 1);  // the block's
  const int kc0 = c * XC;
  if (kc0 > bend) return;  // block-uniform: nothing read, nothing written
  const int klast = min(kc0 + XC - 1, bend);
  const bool active = rw < R;                                                 // wave-uniform
  const int wlo = min(len + min(rw, R - 1) / G, cap - 1);                     // the wave's smallest bound
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
  float m_i = kSplitNoMax, l_i = 0.f;

  const int nkt = (klast - kc0) / KT + 1;  // tiles of this chunk: 1 .. XC / 64
  const int nvalid = bend + 1;             // rows of the cache the block may load (<= min(len + nt, cap))

  Stage<T, D, KT, NW * 64> sk, sv;
  sk.load(Kb, ldkv, kc0, nvalid);
  sv.load(Vb, ldkv, kc0, nvalid);
  sk.store(smem);
  sv.store(smem + TILE);
  __syncthreads();

  auto body = [&](auto cc, int j) {
    constexpr int CUR = decltype(cc)::value;
    const T* Kt = smem + 2 * CUR * TILE;
    const T* Vt = Kt + TILE;
    const int k0 = kc0 + j * KT;
    const bool more = j + 1 < nkt;
    if (more) {
      sk.load(Kb, ldkv, k0 + KT, nvalid);
      sv.load(Vb, ldkv, k0 + KT, nvalid);
    }
    if (j % WS == kw && k0 <= whi) {  // wave-uniform: the wave's tile, and not wholly after its rows' bounds
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
  for (int j = 0; j < nkt; j += 2) {
    body(IC<0>{}, j);
    if (j + 1 < nkt) body(IC<1>{}, j + 1);
  }

  // The waves of a sub-tile, in wave order. The last body ended on a barrier: the tile buffers are free.
  // State slot (sub, kw - 1), word v, lane: consecutive lanes 16 B apart. A wave that took no tile (or has no
  // real row) holds (kSplitNoMax, 0, 0) and folds in with weight exp2(-1e30 - m) = 0, or 1 onto zeros.
  if constexpr (WS > 1) {
    float4* st4 = reinterpret_cast<float4*>(smem);
    if (kw > 0) {
      float4* p = st4 + (long)((sub * (WS - 1) + kw - 1) * NV) * 64 + lane;
#pragma unroll
      for (int i = 0; i < NDB; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q)
          p[(4 * i + q) * 64] = make_float4(o[i][4 * q], o[i][4 * q + 1], o[i][4 * q + 2], o[i][4 * q + 3]);
      p[4 * NDB * 64] = make_float4(m_i, l_i, 0.f, 0.f);
    }
    __syncthreads();
    if (kw == 0) {
#pragma unroll
      for (int w = 1; w < WS; ++w) {
        const float4* p = st4 + (long)((sub * (WS - 1) + w - 1) * NV) * 64 + lane;
        const float4 ml = p[4 * NDB * 64];
        const float m_new = fmaxf(m_i, ml.x);
        const float fa = fexp2(m_i - m_new), fb = fexp2(ml.x - m_new);
        l_i = fmaf(ml.y, fb, l_i * fa);
#pragma unroll
        for (int i = 0; i < NDB; ++i)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float4 x = p[(4 * i + q) * 64];
            o[i][4 * q] = fmaf(x.x, fb, o[i][4 * q] * fa);
            o[i][4 * q + 1] = fmaf(x.y, fb, o[i][4 * q + 1] * fa);
            o[i][4 * q + 2] = fmaf(x.z, fb, o[i][4 * q + 2] * fa);
            o[i][4 * q + 3] = fmaf(x.w, fb, o[i][4 * q + 3] * fa);
          }
        m_i = m_new;
      }
    }
  }

  // a row whose own bound lies before the chunk has no partial here, and the combine reads none
  if (kw == 0 && row < R && kend >= kc0) {
    const long prow = (((long)b * nt + t) * Hq + hq) * NC + c;
    store_rows16_f32<NDB>(o, 1.f, WO + prow * D, h2);
    if (h2 == 0) *reinterpret_cast<float2*>(WML + prow * 2) = make_float2(m_i, l_i);
  }
}

// One output row (sequence, token, head) per D / 4 lanes, 4 columns each; 256 / (D / 4) consecutive rows per
// block, so the heads of a token share blocks. Chunks 0 .. kend / XC in ascending order, kend recomputed as
// the chunk kernel does; chunk 0 holds key 0, so L > 0. No partial of a later chunk is read.
template <typename T, int D>
__global__ __launch_bounds__(256) void extend_combine_kernel(const float* __restrict__ WO, const float* __restrict__ WML,
                                                             const int* __restrict__ KVLEN, T* __restrict__ O,
                                                             float* __restrict__ LSE, long nrows, int nt, int Hq,
                                                             int cap, int NC) {
  constexpr int LPR = D / 4, RPB = 256 / LPR, XC = kExtendChunk;
  const int j = threadIdx.x % LPR;
  const long row = (long)blockIdx.x * RPB + threadIdx.x / LPR;
  if (row >= nrows) return;
  const long bt = row / Hq;
  const int b = (int)(bt / nt), t = (int)(bt - (long)b * nt);
  const int len = min(max(KVLEN[b], 0), cap);
  const int kend = min(len + t, cap - 1);
  const int nc = kend / XC + 1;  // <= NC
  const float2* ml = reinterpret_cast<const float2*>(WML + row * NC * 2);
  const float* po = WO + row * NC * D + 4 * j;
  float M = kSplitNoMax;
  for (int c = 0; c < nc; ++c) M = fmaxf(M, ml[c].x);
  float L = 0.f;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
  for (int c = 0; c < nc; ++c) {
    const float2 s = ml[c];
    const float4 x = *reinterpret_cast<const float4*>(po + (long)c * D);
    const float w = fexp2(s.x - M);
    L = fmaf(s.y, w, L);
    acc.x = fmaf(x.x, w, acc.x);
    acc.y = fmaf(x.y, w, acc.y);
    acc.z = fmaf(x.z, w, acc.z);
    acc.w = fmaf(x.w, w, acc.w);
  }
  const float inv = 1.f / L;
  *reinterpret_cast<uint2*>(O + row * D + 4 * j) =
      make_uint2(pack_x2<T>(acc.x * inv, acc.y * inv), pack_x2<T>(acc.z * inv, acc.w * inv));
  if (j == 0) LSE[row] = (M + __log2f(L)) * 0.69314718055994531f;
}

using WaveSplit = One<1, 2, 4>;

// attention_extend.hip has checked the shape; ws holds pl.ws_floats fp32 words, 16-B aligned
hipError_t extend_split(int dtype, const void* q, long ldq, const void* k_cache, const void* v_cache,
                        const int* kv_len, void* o, float* lse, float* ws, int B, int T, int Hq, int Hkv, int D,
                        int cap, const pra_attn_extend_plan_t& pl, float scale_log2, hipStream_t s) {
  const long nrows = (long)B * T * Hq;
  if (ws == nullptr || pl.blocks > 0x7fffffffL || nrows > 0x7fffffffL || (reinterpret_cast<uintptr_t>(ws) & 15))
    return hipErrorInvalidValue;
  const int NC = pl.chunks;
  float* ws_o = ws;
  float* ws_ml = ws + nrows * NC * D;
  return dispatch_16bit(dtype, [&](auto t) {
    using E = decltype(t);
    const bool found = pra::dispatch(
        [&](auto d, auto w) {
          hipLaunchKernelGGL((extend_split_kernel<E, d(), w()>), dim3((unsigned)pl.blocks), dim3(256), 0, s,
                             (const E*)q, (const E*)k_cache, (const E*)v_cache, ws_o, ws_ml, kv_len, T, Hq, Hkv, cap, NC,
                             ldq, scale_log2);
          constexpr int RPB = 256 / (d() / 4);
          hipLaunchKernelGGL((extend_combine_kernel<E, d()>), dim3((unsigned)((nrows + RPB - 1) / RPB)), dim3(256), 0,
                             s, ws_o, ws_ml, kv_len, (E*)o, lse, nrows, T, Hq, cap, NC);
        },
        HeadDim{D}, WaveSplit{pl.ws_waves});
    return found ? hipGetLastError() : hipErrorInvalidValue;
  });
}

}  // namespace attn
}  // namespace pra

// The merge of the key split alone (attention_extend_fp8.hip writes the same partials). extend_split above keeps its
// own launch of the same kernel beside the chunk kernel's: the two instantiate in one lambda, and that fixes the
// order of the kernels in the code object, which is kept as it was. ws_o [B][T][Hq][NC][D],
// ws_ml [B][T][Hq][NC][2], NC = ceil(cap / kExtendChunk)
extern "C" hipError_t pra_attn_extend_combine(int dtype, const float* ws_o, const float* ws_ml, const int* kv_len,
                                              void* o, float* lse, int B, int T, int Hq, int D, int cap, int NC,
                                              hipStream_t s) {
  using namespace pra::attn;
  const long nrows = (long)B * T * Hq;
  if (ws_o == nullptr || ws_ml == nullptr || kv_len == nullptr || o == nullptr || lse == nullptr || nrows <= 0 ||
      nrows > 0x7fffffffL || NC != (cap + kExtendChunk - 1) / kExtendChunk)
    return hipErrorInvalidValue;
  return dispatch_16bit(dtype, [&](auto t) {
    using E = decltype(t);
    const bool found = pra::dispatch(
        [&](auto d) {
          constexpr int RPB = 256 / (d() / 4);
          hipLaunchKernelGGL((extend_combine_kernel<E, d()>), dim3((unsigned)((nrows + RPB - 1) / RPB)), dim3(256), 0,
                             s, ws_o, ws_ml, kv_len, (E*)o, lse, nrows, T, Hq, cap, NC);
        },
        HeadDim{D});
    return found ? hipGetLastError() : hipErrorInvalidValue;
  });
}
