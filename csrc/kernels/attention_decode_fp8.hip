// fp8 KV cache for generation: the quantizing stores and the decode kernel over an fp8 cache
// (bf16 / fp16 queries, head_dim 64 / 128). The 16-bit kernels of attention_decode.hip are untouched;
// this file reuses their decomposition, their workspace layout and their combine kernel.
//
// Format (a bit contract; ops/reference.py kv_quantize_ref is the torch statement of it). A cache row
// is the D values of one (sequence, position, kv head): D bytes of OCP e4m3fn plus one fp32 scale that
// is an exact power of two. Per layer: k, v uint8 [B][cap][Hkv][D]; k_scale, v_scale fp32 [B][cap][Hkv].
//   amax = max |x_i| over the row (fp32; 16-bit inputs convert exactly)
//   amax == 0: scale 1, bytes 0. Otherwise (m, k) = frexp(amax), m in [0.5, 1),
//   e = clamp(k - 9 + (m > 0.875), -126, 127): the smallest e with amax * 2^-e <= 448 = 0.875 * 2^9
//   byte_i = e4m3fn_rne(x_i * 2^-e)  (the product is exact: one rounding, nothing above 448)
//   dequantized value = byte_i * 2^e, exact in fp32, bf16 and fp16 (e4m3 has 3 mantissa bits)
// Rows with non-finite values are outside the contract: they store something and touch no other row.
//
//   kv_quantize      prefill: the k and v views [B][S][Hkv][D] of the fused QKV activation into cache
//                    rows 0 .. S - 1
//   rope_append_fp8  rope_append_kernel with a quantizing store: q rotated in place (bit-equal), the k
//                    row rotated in fp32, rounded once to the model dtype and then quantized, the v row
//                    quantized from its 16-bit values: the cache is a pure function of what the 16-bit
//                    cache would hold
//   attn_decode_fp8  attn_decode_chunk_kernel over bytes: a 16-B load covers 16 columns, so D / 16
//                    lanes cover a row. K bytes become 16-bit pairs (exact) for the packed dot with fp32
//                    accumulate; the row's K scale multiplies the fp32 score, the V scale the
//                    probability (both exact: powers of two); V bytes become fp32 for the FMA. Same
//                    fp32 partials, same fixed summation order, no atomics; a key at or beyond kv_len[b]
//                    is never loaded, neither its bytes nor its scales.
// In the two storing kernels the D / 8 lanes of a head row are contiguous and aligned in the work-item
// index, and the loops step whole waves, so the amax shuffles are wave-uniform.
#include "common.h"

#include <math.h>

extern "C" {
int pra_attn_decode_chunk();
hipError_t pra_attn_decode_combine(int dtype, const float* ws_o, const float* ws_ml, const int* kv_len, void* o,
                                   float* lse, int B, int Hq, int D, int cap, int NC, hipStream_t s);
}

namespace pra {

// Keys per chunk. The partials go through attention_decode.hip's combine kernel, which derives a
// sequence's chunk count from its own chunk length: the two must be equal (the launcher checks).
// Measured (profiles/decode/README.md): a workgroup that serves two consecutive chunks, i.e. as many bytes
// as a 16-bit chunk, is slower at both shapes, so a workgroup serves one chunk here too.
constexpr int kKC8 = 256;
static_assert(kKC8 % 128 == 0, "chunk length");
constexpr int kDec8Waves = 8;
constexpr int kDec8Threads = 64 * kDec8Waves;
constexpr float kDec8NoMax = -1e30f;  // as kDecNoMax

typedef __bf16 q8_bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 q8_f16x2 __attribute__((ext_vector_type(2)));
typedef float q8_f32x2 __attribute__((ext_vector_type(2)));

// the rule's exponent from the row's amax (>= 0; frexp on the bits)
__device__ __forceinline__ int kv_scale_exp(float amax) {
  const uint32_t bits = __float_as_uint(amax) & 0x7fffffffu;
  if (bits == 0u) return 0;
  const int E = (int)(bits >> 23);
  if (E == 0) return -126;  // subnormal amax: k <= -126, so k - 9 is below the clamp
  // amax = 1.f * 2^(E - 127) = m * 2^k with k = E - 126; m > 0.875 <=> the fraction field > 0.75
  const int e = E - 135 + ((bits & 0x7fffffu) > 0x600000u ? 1 : 0);
  return min(max(e, -126), 127);
}
__device__ __forceinline__ float kv_scale_of(int e) { return __uint_as_float((uint32_t)(e + 127) << 23); }

__device__ __forceinline__ float amax8(const float (&x)[8]) {
  float a = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) a = fmaxf(a, fabsf(x[i]));
  return a;
}
// max over the lph (8 or 16) aligned neighbouring lanes of a head row; every lane of the wave calls it
__device__ __forceinline__ float group_amax(float a, int lph) {
  for (int o = 1; o < lph; o <<= 1) a = fmaxf(a, __shfl_xor(a, o, 64));
  return a;
}
// 8 values * 2^-e (exact) to 8 e4m3fn bytes, round to nearest even. amax == 0: every byte 0x00, also for -0.0
__device__ __forceinline__ uint2 kv_quant8(const float (&x)[8], int e, float amax) {
  float y[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) y[i] = amax == 0.f ? 0.f : ldexpf(x[i], -e);
  int lo = 0, hi = 0;
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], lo, false);
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], lo, true);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(y[4], y[5], hi, false);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(y[6], y[7], hi, true);
  return make_uint2((uint32_t)lo, (uint32_t)hi);
}

// k, v [B * S][ld] views (Hkv * D columns each); one lane per 8 columns, k rows first, then v rows.
template <typename T>
__global__ __launch_bounds__(256) void kv_quantize_kernel(const T* __restrict__ k, const T* __restrict__ v,
                                                          uint8_t* __restrict__ kq, uint8_t* __restrict__ vq,
                                                          float* __restrict__ ks, float* __restrict__ vs, int B, int S,
                                                          long ld, int Hkv, int D, int cap) {
  const int lph = D / 8;
  const int vpt = Hkv * lph;  // 16-B vectors per token of one tensor
  const long per = (long)B * S * vpt;
  const long total = 2 * per;
  const int lane = threadIdx.x & 63;
  for (long base = (long)blockIdx.x * 256 + (threadIdx.x - lane); base < total; base += (long)gridDim.x * 256) {
    const long idx = base + lane;
    const bool live = idx < total;  // a head row's lanes are all live or all not
    float x[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    bool isv = false;
    long tok = 0;
    int c = 0;
    if (live) {
      isv = idx >= per;
      const long rem = idx - (isv ? per : 0);
      tok = rem / vpt;
      c = (int)(rem - tok * vpt);
      load8<T>((isv ? v : k) + tok * ld + c * 8, x);
    }
    const float amax = group_amax(amax8(x), lph);
    const int e = kv_scale_exp(amax);
    if (live) {
      const long b = tok / S;
      const long row = b * cap + (tok - b * S);
      *reinterpret_cast<uint2*>((isv ? vq : kq) + row * Hkv * D + c * 8) = kv_quant8(x, e, amax);
      if (c % lph == 0) (isv ? vs : ks)[row * Hkv + c / lph] = kv_scale_of(e);
    }
  }
}

// (a + ib) * (c + is): rope_append_kernel's dec_rot_pair, which is elementwise.hip's rot_pair
__device__ __forceinline__ void q8_rot_pair(float a, float b, float c, float s, float& o0, float& o1) {
  o0 = __builtin_fmaf(a, c, -(b * s));
  o1 = __builtin_fmaf(a, s, b * c);
}

// qkv [B][ld]: q (Hq heads) | k (Hkv) | v (Hkv), D columns each. One lane per 8 columns.
template <typename T>
__global__ __launch_bounds__(256) void rope_append_fp8_kernel(T* __restrict__ qkv, const float2* __restrict__ tab,
                                                              const int* __restrict__ kv_len, uint8_t* __restrict__ kq,
                                                              uint8_t* __restrict__ vq, float* __restrict__ ks,
                                                              float* __restrict__ vs, int B, long ld, int Hq, int Hkv,
                                                              int D, int cap) {
  const int nq = Hq * D, nk = Hkv * D;
  const int lph = D / 8;
  const int vpr = (nq + 2 * nk) / 8;  // a multiple of lph
  const long total = (long)B * vpr;
  const int lane = threadIdx.x & 63;
  for (long base = (long)blockIdx.x * 256 + (threadIdx.x - lane); base < total; base += (long)gridDim.x * 256) {
    const long idx = base + lane;
    const bool live = idx < total;
    float x[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};  // what this lane quantizes (k, v lanes)
    int kind = 0;                                            // 1: k row, 2: v row
    long row = 0;
    int cin = 0;  // column inside the k (or v) part
    if (live) {
      const int b = (int)(idx / vpr);
      const int col = (int)(idx - (long)b * vpr) * 8;
      const int pos = min(max(kv_len[b], 0), cap - 1);
      T* p = qkv + (long)b * ld + col;
      float v[8];
      load8<T>(p, v);
      row = (long)b * cap + pos;
      if (col >= nq + nk) {
        kind = 2;
        cin = col - nq - nk;
#pragma unroll
        for (int i = 0; i < 8; ++i) x[i] = v[i];
      } else {
        const int pi = (col % D) / 2;
        const float4* tp = reinterpret_cast<const float4*>(tab + (size_t)pos * (D / 2) + pi);
        const float4 cs01 = tp[0], cs23 = tp[1];
        const float c[4] = {cs01.x, cs01.z, cs23.x, cs23.z};
        const float s[4] = {cs01.y, cs01.w, cs23.y, cs23.w};
        float o[8];
#pragma unroll
        for (int j = 0; j < 4; ++j) q8_rot_pair(v[2 * j], v[2 * j + 1], c[j], s[j], o[2 * j], o[2 * j + 1]);
        if (col < nq) {
          store8<T>(p, o);
        } else {
          kind = 1;
          cin = col - nq;
#pragma unroll
          for (int i = 0; i < 8; ++i) x[i] = rnd<T>(o[i]);  // what the 16-bit cache would hold
        }
      }
    }
    const float amax = group_amax(amax8(x), lph);
    const int e = kv_scale_exp(amax);
    if (kind != 0) {
      *reinterpret_cast<uint2*>((kind == 2 ? vq : kq) + row * nk + cin) = kv_quant8(x, e, amax);
      if (cin % D == 0) (kind == 2 ? vs : ks)[row * Hkv + cin / D] = kv_scale_of(e);
    }
  }
}

// 16 columns of q (two 16-B loads of 16-bit pairs) against 16 e4m3fn bytes of a K row: the bytes become
// 16-bit pairs (exact; scale operand 1) and go through the packed dot with fp32 accumulate.
template <typename T>
__device__ __forceinline__ float dot16(const uint4& qa, const uint4& qb, const uint4& kb);
template <>
__device__ __forceinline__ float dot16<__bf16>(const uint4& qa, const uint4& qb, const uint4& kb) {
  const uint32_t qw[8] = {qa.x, qa.y, qa.z, qa.w, qb.x, qb.y, qb.z, qb.w};
  const uint32_t kw[4] = {kb.x, kb.y, kb.z, kb.w};
  float c = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const q8_bf16x2 lo = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)kw[j], 1.0f, false);
    const q8_bf16x2 hi = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)kw[j], 1.0f, true);
    c = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(q8_bf16x2, qw[2 * j]), lo, c, false);
    c = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(q8_bf16x2, qw[2 * j + 1]), hi, c, false);
  }
  return c;
}
template <>
__device__ __forceinline__ float dot16<__half>(const uint4& qa, const uint4& qb, const uint4& kb) {
  const uint32_t qw[8] = {qa.x, qa.y, qa.z, qa.w, qb.x, qb.y, qb.z, qb.w};
  const uint32_t kw[4] = {kb.x, kb.y, kb.z, kb.w};
  float c = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const q8_f16x2 lo = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)kw[j], 1.0f, false);
    const q8_f16x2 hi = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)kw[j], 1.0f, true);
    c = __builtin_amdgcn_fdot2(__builtin_bit_cast(q8_f16x2, qw[2 * j]), lo, c, false);
    c = __builtin_amdgcn_fdot2(__builtin_bit_cast(q8_f16x2, qw[2 * j + 1]), hi, c, false);
  }
  return c;
}

// 8 e4m3fn bytes (two words) as fp32 (exact); zeros for a key that was never loaded
__device__ __forceinline__ void unpack8_fp8(uint32_t w0, uint32_t w1, float (&o)[8]) {
  const uint32_t w[2] = {w0, w1};
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const q8_f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[j], false);
    const q8_f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[j], true);
    o[4 * j] = lo.x;
    o[4 * j + 1] = lo.y;
    o[4 * j + 2] = hi.x;
    o[4 * j + 3] = hi.y;
  }
}

// Partials as attn_decode_chunk_kernel: ws_o [B][Hq][NC][D] fp32 (unnormalised), ws_ml [B][Hq][NC][2].
// grid (NC, Hkv * (G / GT), B). LPK = D / 16 lanes cover one cache row (16 B each), the workgroup's 8
// waves cover KPB = 8 * 64 / LPK consecutive rows per step, and a lane issues the loads of all its K and
// V rows of the chunk (kKC8 / KPB each) before the first use. The first lane of a row also loads the
// row's two scales: the K scale multiplies the score it writes, the V scale is parked in LDS beside the
// score and folded into the probability (p * 2^e_v, exact) by the softmax phase.
template <typename T, int D, int GT>
__global__ __launch_bounds__(kDec8Threads) void attn_decode_fp8_chunk_kernel(
    const T* __restrict__ q, const uint8_t* __restrict__ kc, const uint8_t* __restrict__ vc,
    const float* __restrict__ ksc, const float* __restrict__ vsc, const int* __restrict__ kv_len,
    float* __restrict__ ws_o, float* __restrict__ ws_ml, int Hq, int Hkv, int cap, int NC, float scale_log2) {
  constexpr int LPK = D / 16;
  constexpr int KPW = 64 / LPK;
  constexpr int KPB = kDec8Waves * KPW;
  constexpr int STEPS = kKC8 / KPB;  // rows of K (and of V) per lane
  static_assert(kKC8 % KPB == 0 && STEPS >= 1, "chunk must tile");
  __shared__ float s_p[kKC8 * GT];              // [key][g]: scores, then probabilities * V scale
  __shared__ float s_vs[kKC8];                  // [key]: V scale (0 for a masked key)
  __shared__ float s_red[kDec8Waves * GT * D];  // [wave][g][d]: per-wave P.V

  const int b = blockIdx.z;
  const int G = Hq / Hkv;
  const int tiles = G / GT;
  const int hkv = blockIdx.y / tiles;
  const int h0 = hkv * G + (blockIdx.y - hkv * tiles) * GT;  // first query head served here
  const int chunk = blockIdx.x;
  const int len = min(max(kv_len[b], 0), cap);
  const int c0 = chunk * kKC8;
  if (c0 >= len) return;  // wave-uniform: nothing read, nothing written

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int part = lane % LPK;  // which 16 columns of the row
  const int ks = lane / LPK;    // which row of the wave-load
  const long tok_stride = (long)Hkv * D;
  const uint8_t* kbase = kc + ((long)b * cap + c0) * tok_stride + (long)hkv * D + part * 16;
  const uint8_t* vbase = vc + ((long)b * cap + c0) * tok_stride + (long)hkv * D + part * 16;
  const long sbase = ((long)b * cap + c0) * Hkv + hkv;

  // every load of the chunk, K first; a key at or beyond len is never loaded (zeros stand in)
  uint4 kraw[STEPS], vraw[STEPS];
  float kscale[STEPS], vscale[STEPS];
#pragma unroll
  for (int st = 0; st < STEPS; ++st) {
    const int kl = st * KPB + wave * KPW + ks;  // key within the chunk
    kraw[st] = make_uint4(0u, 0u, 0u, 0u);
    kscale[st] = 0.f;
    if (c0 + kl < len) {
      kraw[st] = *reinterpret_cast<const uint4*>(kbase + (long)kl * tok_stride);
      if (part == 0) kscale[st] = ksc[sbase + (long)kl * Hkv];
    }
  }
#pragma unroll
  for (int st = 0; st < STEPS; ++st) {
    const int kl = st * KPB + wave * KPW + ks;
    vraw[st] = make_uint4(0u, 0u, 0u, 0u);
    vscale[st] = 0.f;
    if (c0 + kl < len) {
      vraw[st] = *reinterpret_cast<const uint4*>(vbase + (long)kl * tok_stride);
      if (part == 0) vscale[st] = vsc[sbase + (long)kl * Hkv];
    }
  }

  // ---- phase 1: scores ---------------------------------------------------------------
  {
    uint4 qa[GT], qb[GT];
#pragma unroll
    for (int g = 0; g < GT; ++g) {
      const uint4* qp = reinterpret_cast<const uint4*>(q + ((long)b * Hq + h0 + g) * D + part * 16);
      qa[g] = qp[0];
      qb[g] = qp[1];
    }
#pragma unroll
    for (int st = 0; st < STEPS; ++st) {
      const int kl = st * KPB + wave * KPW + ks;
      float d[GT];
#pragma unroll
      for (int g = 0; g < GT; ++g) d[g] = dot16<T>(qa[g], qb[g], kraw[st]);
#pragma unroll
      for (int o = 1; o < LPK; o <<= 1) {
#pragma unroll
        for (int g = 0; g < GT; ++g) d[g] += __shfl_xor(d[g], o, 64);
      }
      if (part == 0) {
        const bool valid = c0 + kl < len;
        const float f = kscale[st] * scale_log2;
#pragma unroll
        for (int g = 0; g < GT; ++g) s_p[kl * GT + g] = valid ? d[g] * f : -INFINITY;
        s_vs[kl] = vscale[st];
      }
    }
  }
  __syncthreads();

  // ---- phase 2: per head, exact max, probabilities, their sum (one wave per head)
  for (int g = wave; g < GT; g += kDec8Waves) {
    float sv[kKC8 / 64];
    float m = kDec8NoMax;
#pragma unroll
    for (int i = 0; i < kKC8 / 64; ++i) {
      sv[i] = s_p[(i * 64 + lane) * GT + g];
      m = fmaxf(m, sv[i]);
    }
    m = wave_max(m);
    float l = 0.f;
#pragma unroll
    for (int i = 0; i < kKC8 / 64; ++i) {
      const float p = exp2f(sv[i] - m);  // masked key: exp2(-inf) = 0, m is finite
      s_p[(i * 64 + lane) * GT + g] = p * s_vs[i * 64 + lane];
      l += p;
    }
    l = wave_sum(l);
    if (lane == 0) {
      float* ml = ws_ml + (((long)b * Hq + h0 + g) * NC + chunk) * 2;
      ml[0] = m;
      ml[1] = l;
    }
  }
  __syncthreads();

  // ---- phase 3: P.V, 8 of the lane's 16 columns at a time (half the accumulators live at once) ----
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    float acc[GT][8];
#pragma unroll
    for (int g = 0; g < GT; ++g)
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[g][i] = 0.f;
#pragma unroll
    for (int st = 0; st < STEPS; ++st) {
      const int kl = st * KPB + wave * KPW + ks;
      float vf[8];
      unpack8_fp8(half ? vraw[st].z : vraw[st].x, half ? vraw[st].w : vraw[st].y, vf);  // zeros for a masked key
#pragma unroll
      for (int g = 0; g < GT; ++g) {
        const float p = s_p[kl * GT + g];
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[g][i] = __builtin_fmaf(p, vf[i], acc[g][i]);
      }
    }
    // rows of the wave-load (lanes with the same `part`), then the waves in order
#pragma unroll
    for (int o = LPK; o < 64; o <<= 1) {
#pragma unroll
      for (int g = 0; g < GT; ++g)
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[g][i] += __shfl_xor(acc[g][i], o, 64);
    }
    if (ks == 0) {
#pragma unroll
      for (int g = 0; g < GT; ++g)
#pragma unroll
        for (int i = 0; i < 8; ++i) s_red[(wave * GT + g) * D + part * 16 + half * 8 + i] = acc[g][i];
    }
  }
  __syncthreads();
  for (int e = tid; e < GT * D; e += kDec8Threads) {
    const int g = e / D, dcol = e - g * D;
    float s = s_red[e];
#pragma unroll
    for (int w = 1; w < kDec8Waves; ++w) s += s_red[w * GT * D + e];
    ws_o[(((long)b * Hq + h0 + g) * NC + chunk) * D + dcol] = s;
  }
}

template <typename T, int D, int GT>
static hipError_t launch_chunks_fp8(const void* q, const void* kc, const void* vc, const float* ksc, const float* vsc,
                                    const int* kv_len, float* ws_o, float* ws_ml, int B, int Hq, int Hkv, int cap,
                                    int NC, float scale, hipStream_t st) {
  const int tiles = (Hq / Hkv) / GT;
  hipLaunchKernelGGL((attn_decode_fp8_chunk_kernel<T, D, GT>), dim3(NC, Hkv * tiles, B), dim3(kDec8Threads), 0, st,
                     (const T*)q, (const uint8_t*)kc, (const uint8_t*)vc, ksc, vsc, kv_len, ws_o, ws_ml, Hq, Hkv, cap,
                     NC, scale * 1.4426950408889634f);
  return hipGetLastError();
}

template <typename T, int D>
static hipError_t launch_decode_fp8(const void* q, const void* kc, const void* vc, const float* ksc, const float* vsc,
                                    const int* kv_len, float* ws_o, float* ws_ml, int B, int Hq, int Hkv, int cap,
                                    int NC, float scale, hipStream_t st) {
  const int G = Hq / Hkv;
  // the widest head tile that divides the group, as the 16-bit kernel
  if (G % 8 == 0) return launch_chunks_fp8<T, D, 8>(q, kc, vc, ksc, vsc, kv_len, ws_o, ws_ml, B, Hq, Hkv, cap, NC, scale, st);
  if (G % 4 == 0) return launch_chunks_fp8<T, D, 4>(q, kc, vc, ksc, vsc, kv_len, ws_o, ws_ml, B, Hq, Hkv, cap, NC, scale, st);
  if (G % 2 == 0) return launch_chunks_fp8<T, D, 2>(q, kc, vc, ksc, vsc, kv_len, ws_o, ws_ml, B, Hq, Hkv, cap, NC, scale, st);
  return launch_chunks_fp8<T, D, 1>(q, kc, vc, ksc, vsc, kv_len, ws_o, ws_ml, B, Hq, Hkv, cap, NC, scale, st);
}

}  // namespace pra

extern "C" {

int pra_attn_decode_fp8_chunk() { return pra::kKC8; }

hipError_t pra_kv_quantize(int dtype, const void* k, const void* v, long ld, void* k_cache, void* v_cache,
                           float* k_scale, float* v_scale, int B, int S, int Hkv, int D, int cap, hipStream_t s) {
  if (B <= 0 || S <= 0 || S > cap || Hkv <= 0 || (D != 64 && D != 128) || ld % 8 || ld < (long)Hkv * D)
    return hipErrorInvalidValue;
  const long items = 2L * B * S * Hkv * D / 8;
  long grid = (items + 255) / 256;
  if (grid > 4096) grid = 4096;
  PRA_DISPATCH_16BIT(dtype, T,
                     hipLaunchKernelGGL((pra::kv_quantize_kernel<T>), dim3((unsigned)grid), dim3(256), 0, s,
                                        (const T*)k, (const T*)v, (uint8_t*)k_cache, (uint8_t*)v_cache, k_scale,
                                        v_scale, B, S, ld, Hkv, D, cap));
  return hipGetLastError();
}

hipError_t pra_rope_append_fp8(int dtype, void* qkv, const void* tab, const int* kv_len, void* k_cache, void* v_cache,
                               float* k_scale, float* v_scale, int B, long ld, int Hq, int Hkv, int D, int cap,
                               hipStream_t s) {
  if (B <= 0 || cap <= 0 || Hq <= 0 || Hkv <= 0 || (D != 64 && D != 128) || ld % 8) return hipErrorInvalidValue;
  const long items = (long)B * (Hq + 2 * Hkv) * D / 8;
  long grid = (items + 255) / 256;
  if (grid > 2048) grid = 2048;
  PRA_DISPATCH_16BIT(dtype, T,
                     hipLaunchKernelGGL((pra::rope_append_fp8_kernel<T>), dim3((unsigned)grid), dim3(256), 0, s,
                                        (T*)qkv, (const float2*)tab, kv_len, (uint8_t*)k_cache, (uint8_t*)v_cache,
                                        k_scale, v_scale, B, ld, Hq, Hkv, D, cap));
  return hipGetLastError();
}

hipError_t pra_attn_decode_fp8(int dtype, const void* q, const void* k_cache, const void* v_cache,
                               const float* k_scale, const float* v_scale, const int* kv_len, void* o, float* lse,
                               float* ws, int B, int Hq, int Hkv, int D, int cap, float scale, hipStream_t s) {
  if (B <= 0 || cap <= 0 || Hkv <= 0 || Hq % Hkv || B > 65535 || Hq > 65535) return hipErrorInvalidValue;
  if (pra_attn_decode_chunk() != pra::kKC8) return hipErrorInvalidValue;  // the shared combine kernel's chunking
  const int NC = (cap + pra::kKC8 - 1) / pra::kKC8;
  float* ws_o = ws;
  float* ws_ml = ws + (long)B * Hq * NC * D;
  hipError_t e = hipErrorInvalidValue;
  PRA_DISPATCH_16BIT(dtype, T, {
    if (D == 64)
      e = pra::launch_decode_fp8<T, 64>(q, k_cache, v_cache, k_scale, v_scale, kv_len, ws_o, ws_ml, B, Hq, Hkv, cap, NC, scale, s);
    else if (D == 128)
      e = pra::launch_decode_fp8<T, 128>(q, k_cache, v_cache, k_scale, v_scale, kv_len, ws_o, ws_ml, B, Hq, Hkv, cap, NC, scale, s);
  });
  if (e != hipSuccess) return e;
  return pra_attn_decode_combine(dtype, ws_o, ws_ml, kv_len, o, lse, B, Hq, D, cap, NC, s);
}
}
