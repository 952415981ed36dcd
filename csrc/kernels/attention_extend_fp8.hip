// Multi-token KV-cache append ("extend") attention over an fp8 cache for gfx950: bf16 / fp16 queries,
// head_dim 64 / 128, native GQA. attention_extend.hip and attention_extend_split.hip with one difference: how K
// and V reach the MFMAs.
//
// The cache (attention_decode_fp8.hip documents the format): k, v uint8 [B][cap][Hkv][D] of e4m3fn bytes,
// k_scale, v_scale fp32 [B][cap][Hkv], exact powers of two. The T new tokens' rows are in the cache already
// (rope_append_fp8 with T tokens runs first): query t of sequence b attends to the DEQUANTIZED rows
// 0 .. min(kv_len[b] + t, cap - 1), its own and the other new rows included. The cache is the single
// source of K and V, as for a decode step.
//
// Staging (Stage8). A 64-key tile is 64 x D bytes, half the 16-bit tile: one (D 64) or two (D 128) 16-B
// loads per thread for K and the same for V. A lane's 16 B lie in one cache row, so the lane loads that
// row's scale itself (the D / 16 lanes of a row read one address). Between the global load and the LDS
// store the bytes are converted in registers by v_cvt_scalef32_pk_{bf16,f16}_fp8 with the row's scale as
// the scale operand, so what lands in LDS is the dequantized tile in the swizzled 16-bit image of
// attn_common.h (Stage::store's): every byte is converted once per block, never per MFMA operand read,
// and LaneOff::rowk / the transposed ds_read_b64_tr_b16 reads of V work as they are. Both scales are folded
// into the values for both dtypes: byte * 2^e is exact in bf16 and in fp16 for every row that
// kv_quantize / rope_append_fp8 wrote from that dtype (the op's results are specified for such caches), so
// no intermediate leaves the dtype's range (P * 2^e_v in fp16 would), and from the LDS image on the kernel
// has the 16-bit kernel's rounding points and no more. A stage holds 2 x (4 + 1) registers per tensor at
// D 128 where the 16-bit stage holds 2 x 8. No native fp8 MFMA: it would need quantized Q and P.
//
// Store lanes: an 8-lane group of a ds_write_b128 takes byte chunks {cb, cb + 1} of rows {r, r + 1, r + 4,
// r + 5}: 16-bit chunks 2 cb + j, j fixed per store, land on 64 (r & 1) + 16 (slot) with the four slots
// distinct (cb's low bit flips slot bit 1, row bit 2 flips slot bit 0 through the image's XOR): 128
// distinct bytes mod 128, conflict-free. A wave's 64 loads cover whole cache rows.
//
// Load bounds are the 16-bit kernel's: nothing at or beyond min(kv_len[b] + T, cap) is loaded, neither
// bytes nor scales; bytes 0 and scale 1 stand in (and are masked). Whatever the tail holds, NaN bytes
// 0x7F / 0xFF and NaN / Inf scales included, cannot reach an output.
//
// One kernel serves both arms. SPLIT = false is the single pass (WS = 1: four 32-row sub-tiles, the block
// walks every key tile of its rows, the row-per-lane epilogue writes o / lse). SPLIT = true is the key
// split: a block belongs to (row tile, kv head, sequence, chunk of kExtendChunk keys), the WS waves (4 / 2
// / 1) that share a 32-row sub-tile divide the chunk's key tiles and fold their states in wave order, and
// the fp32 partial goes to the workspace that attention_extend_split.hip's extend_combine_kernel merges in
// ascending chunk order. The plan is extend_plan (attn_extend_plan.h), unchanged: shapes and CU count only.
// No atomics, one fixed summation order per arm: for a fixed split setting a sequence's o / lse are a pure
// function of its own q, cache rows, kv_len[b] and T, with the same bits from run to run.
// Compiled with -fno-honor-nans like attention_extend.hip: no NaN is formed.
// From the first MFMA on, the kernel body is extend_split_kernel's (and, with SPLIT = false, extend_fwd_kernel's)
// line for line: a copy, because those kernels' device code must stay as it is. A change to the tile loop, the
// wave fold or the partial store goes into all three files.
#include "attn_common.h"
#include "common.h"
#include "attn_launch.h"

namespace pra {
namespace attn {

constexpr float kFp8NoMax = -1e30f;  // attention_extend.hip's kNoMax

typedef __bf16 x8_bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 x8_f16x2 __attribute__((ext_vector_type(2)));

// bytes (2 hi, 2 hi + 1) of word w times sc as a 16-bit pair (exact for the cache's rows)
template <typename T>
__device__ __forceinline__ uint32_t cvt2(uint32_t w, float sc, bool hi);
template <>
__device__ __forceinline__ uint32_t cvt2<__bf16>(uint32_t w, float sc, bool hi) {
  return hi ? __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)w, sc, true))
            : __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)w, sc, false));
}
template <>
__device__ __forceinline__ uint32_t cvt2<_Float16>(uint32_t w, float sc, bool hi) {
  return hi ? __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)w, sc, true))
            : __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)w, sc, false));
}

// Stage a 64 x D tile of bytes and its 64 row scales into registers; store() converts and writes the
// dequantized 16-bit tile into attn_common.h's LDS image. 256 threads.
template <typename T, int D>
struct Stage8 {
  static constexpr int CB = D / 16;       // 16-B byte chunks of a row
  static constexpr int R64 = 64 / CB;     // rows covered by 64 consecutive chunk indices (one wave-load)
  static constexpr int CPT = 64 * CB / 256;
  static_assert(CPT * 256 == 64 * CB, "the tile splits evenly over the block");
  uint4 r[CPT];
  float sc[CPT];
  __device__ __forceinline__ static void rc(int idx, int& row, int& cb) {
    const int l = idx & 63, h = l >> 3, rest = h / (CB / 2);
    cb = (l & 1) + 2 * (h % (CB / 2));
    row = R64 * (idx >> 6) + ((l >> 1) & 1) + 4 * ((l >> 2) & 1) + 2 * (rest & 1) + 8 * (rest >> 1);
  }
  // g: the (sequence, kv head)'s first byte; gs: its first scale; ld: bytes between rows; lds: scales between rows
  __device__ __forceinline__ void load(const uint8_t* g, const float* gs, long ld, int lds, int row0, int nrows_valid) {
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
      int row, cb;
      rc(i * 256 + threadIdx.x, row, cb);
      if (row0 + row < nrows_valid) {
        r[i] = *reinterpret_cast<const uint4*>(g + (long)(row0 + row) * ld + cb * 16);
        sc[i] = gs[(long)(row0 + row) * lds];
      } else {
        r[i] = make_uint4(0, 0, 0, 0);
        sc[i] = 1.f;
      }
    }
  }
  __device__ __forceinline__ void store(T* tile) const {
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
      int row, cb;
      rc(i * 256 + threadIdx.x, row, cb);
      const float s = sc[i];
      const uint4 lo = make_uint4(cvt2<T>(r[i].x, s, false), cvt2<T>(r[i].x, s, true), cvt2<T>(r[i].y, s, false),
                                  cvt2<T>(r[i].y, s, true));
      const uint4 hi = make_uint4(cvt2<T>(r[i].z, s, false), cvt2<T>(r[i].z, s, true), cvt2<T>(r[i].w, s, false),
                                  cvt2<T>(r[i].w, s, true));
      *reinterpret_cast<uint4*>(reinterpret_cast<char*>(tile) + lay_byte<D>(row, 2 * cb)) = lo;
      *reinterpret_cast<uint4*>(reinterpret_cast<char*>(tile) + lay_byte<D>(row, 2 * cb + 1)) = hi;
    }
  }
};

// SPLIT: grid (row tiles x Hkv x B) x NC, the chunk fastest; else grid row tiles x Hkv x B (NC = 1). The row
// tile is slowest and descending: late row tiles walk the most keys. Q rows are [B * nt][ldq]. SPLIT writes
// WO fp32 [B][nt][Hq][NC][D] and WML fp32 [B][nt][Hq][NC][2] = (max, sum); else O [B][nt][Hq][D] and LSE.
template <typename T, int D, int WS, bool SPLIT>
__global__ __launch_bounds__(256, 2) void extend_fp8_kernel(const T* __restrict__ Q, const uint8_t* __restrict__ K,
                                                            const uint8_t* __restrict__ V,
                                                            const float* __restrict__ KS, const float* __restrict__ VS,
                                                            T* __restrict__ O, float* __restrict__ LSE,
                                                            float* __restrict__ WO, float* __restrict__ WML,
                                                            const int* __restrict__ KVLEN, int nt, int Hq, int Hkv,
                                                            int cap, int NC, long ldq, float scale_log2) {
  static_assert(SPLIT || WS == 1, "the single pass has one wave per sub-tile");
  constexpr int NW = 4, KT = 64, NSUB = NW / WS, QT = 32 * NSUB, XC = kExtendChunk;
  constexpr int NKS = D / 16, NDB = D / 32, TILE = KT * D;
  constexpr int NV = 4 * NDB + 1;  // float4 words of one lane's (o, m, l)
  static_assert((NW - NSUB) * NV * 64 * 16 <= 4 * TILE * (int)sizeof(T), "the merged states must fit the tile buffer");
  __shared__ __attribute__((aligned(16))) T smem[4 * TILE];  // K0 V0 K1 V1, dequantized

  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, h2 = lane >> 5, l32 = lane & 31;
  const int sub = wid / WS, kw = wid % WS;  // the wave's 32-row sub-tile, and its share of the key tiles
  const int G = Hq / Hkv, R = nt * G;       // rows r = t * G + g of a (sequence, kv head)
  const int nrt = (R + QT - 1) / QT;
  const int c = SPLIT ? blockIdx.x % NC : 0;
  const int rest = SPLIT ? blockIdx.x / NC : blockIdx.x;
  const int BH = (SPLIT ? gridDim.x / NC : gridDim.x) / nrt;
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
  if (SPLIT && kc0 > bend) return;  // block-uniform: nothing read, nothing written
  const int klast = SPLIT ? min(kc0 + XC - 1, bend) : bend;
  const bool active = rw < R;                                                 // wave-uniform
  const int wlo = min(len + min(rw, R - 1) / G, cap - 1);                     // the wave's smallest bound
  const int whi = active ? min(len + min(rw + 31, R - 1) / G, cap - 1) : -1;  // and its largest

  const long ldkv = (long)Hkv * D;  // bytes
  const uint8_t* Kb = K + (long)b * cap * ldkv + hk * D;
  const uint8_t* Vb = V + (long)b * cap * ldkv + hk * D;
  const float* KSb = KS + (long)b * cap * Hkv + hk;
  const float* VSb = VS + (long)b * cap * Hkv + hk;
  const T* Qr = Q + ((long)b * nt + t) * ldq + hq * D + 8 * h2;

  LaneOff<T, D> lo;
  lo.init(lane);
  V8<T> qf[NKS];
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) qf[ks] = *reinterpret_cast<const V8<T>*>(Qr + 16 * ks);

  f32x16 o[NDB];
#pragma unroll
  for (int i = 0; i < NDB; ++i) o[i] = f32x16{};
  float m_i = kFp8NoMax, l_i = 0.f;

  const int nkt = (klast - kc0) / KT + 1;  // tiles of this block: at least one
  const int nvalid = bend + 1;             // rows of the cache the block may load (<= min(len + nt, cap))

  Stage8<T, D> sk, sv;
  sk.load(Kb, KSb, ldkv, Hkv, kc0, nvalid);
  sv.load(Vb, VSb, ldkv, Hkv, kc0, nvalid);
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
      sk.load(Kb, KSb, ldkv, Hkv, k0 + KT, nvalid);
      sv.load(Vb, VSb, ldkv, Hkv, k0 + KT, nvalid);
    }
    if ((WS == 1 || j % WS == kw) && k0 <= whi) {  // wave-uniform: the wave's tile, not wholly after its rows' bounds
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

  // The waves of a sub-tile, in wave order (attention_extend_split.hip's fold). The last body ended on a
  // barrier: the tile buffers are free. A wave that took no tile holds (kFp8NoMax, 0, 0) and folds in with
  // weight exp2(-1e30 - m) = 0, or 1 onto zeros.
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

  const long orow = ((long)b * nt + t) * Hq + hq;
  if constexpr (SPLIT) {
    // a row whose own bound lies before the chunk has no partial here, and the combine reads none
    if (kw == 0 && row < R && kend >= kc0) {
      const long prow = orow * NC + c;
      store_rows16_f32<NDB>(o, 1.f, WO + prow * D, h2);
      if (h2 == 0) *reinterpret_cast<float2*>(WML + prow * 2) = make_float2(m_i, l_i);
    }
  } else {
    // a real row saw key 0 at least: l_i > 0. A wave without real rows kept l_i = 0 and stores nothing.
    const bool ok = row < R;
    const float inv = l_i > 0.f ? 1.f / l_i : 0.f;
    store_rows16<T, NDB>(o, inv, O + orow * D, ok, h2);  // all 64 lanes: the lane swap
    if (ok && h2 == 0) LSE[orow] = (m_i + __log2f(l_i)) * 0.69314718055994531f;
  }
}

using WaveSplit8 = One<1, 2, 4>;

}  // namespace attn
}  // namespace pra

extern "C" hipError_t pra_attn_extend_fp8(int dtype, const void* q, long ldq, const void* k_cache, const void* v_cache,
                                          const float* k_scale, const float* v_scale, const int* kv_len, void* o,
                                          float* lse, float* ws, int B, int T, int Hq, int Hkv, int D, int cap,
                                          float scale, int split, hipStream_t s) {
  using namespace pra::attn;
  if (q == nullptr || k_cache == nullptr || v_cache == nullptr || k_scale == nullptr || v_scale == nullptr ||
      kv_len == nullptr || o == nullptr || lse == nullptr)
    return hipErrorInvalidValue;
  if (B <= 0 || T <= 0 || cap <= 0 || Hq <= 0 || Hkv <= 0 || Hq % Hkv || (D != 64 && D != 128) || ldq % 8 ||
      ldq < (long)Hq * D || (long)T * (Hq / Hkv) > 0x7fffffffL - 128 || (long)cap > 0x7fffffffL / 2 || split < -1 ||
      split > 1)
    return hipErrorInvalidValue;
  const float sl2 = scale * kLog2e;
  const pra_attn_extend_plan_t pl = extend_plan(B, T, Hq, Hkv, D, cap, device_cus(), split);
  if (pl.blocks > 0x7fffffffL) return hipErrorInvalidValue;
  const dim3 grid((unsigned)pl.blocks), block(256);
  const uint8_t* kc = (const uint8_t*)k_cache;
  const uint8_t* vc = (const uint8_t*)v_cache;
  if (!pl.split)
    return dispatch_16bit(dtype, [&](auto t) {
      using E = decltype(t);
      pra::dispatch(
          [&](auto d) {
            hipLaunchKernelGGL((extend_fp8_kernel<E, d(), 1, false>), grid, block, 0, s, (const E*)q, kc, vc, k_scale,
                               v_scale, (E*)o, lse, (float*)nullptr, (float*)nullptr, kv_len, T, Hq, Hkv, cap, 1, ldq,
                               sl2);
          },
          HeadDim{D});
      return hipGetLastError();
    });
  const long nrows = (long)B * T * Hq;
  if (ws == nullptr || nrows > 0x7fffffffL || (reinterpret_cast<uintptr_t>(ws) & 15)) return hipErrorInvalidValue;
  const int NC = pl.chunks;
  float* ws_o = ws;
  float* ws_ml = ws + nrows * NC * D;
  const hipError_t e = dispatch_16bit(dtype, [&](auto t) {
    using E = decltype(t);
    const bool found = pra::dispatch(
        [&](auto d, auto w) {
          hipLaunchKernelGGL((extend_fp8_kernel<E, d(), w(), true>), grid, block, 0, s, (const E*)q, kc, vc, k_scale,
                             v_scale, (E*)nullptr, (float*)nullptr, ws_o, ws_ml, kv_len, T, Hq, Hkv, cap, NC, ldq, sl2);
        },
        HeadDim{D}, WaveSplit8{pl.ws_waves});
    return found ? hipGetLastError() : hipErrorInvalidValue;
  });
  if (e != hipSuccess) return e;
  return pra_attn_extend_combine(dtype, ws_o, ws_ml, kv_len, o, lse, B, T, Hq, D, cap, NC, s);
}
