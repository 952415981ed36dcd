// MXFP4 KV cache for generation: the quantizing stores and the decode kernel over an fp4 cache
// (bf16 / fp16 queries, head_dim 64 / 128). The 16-bit and fp8 kernels are untouched; this file reuses the
// decomposition, the workspace layout and the combine kernel of attention_decode.hip.
//
// Format (a bit contract; ops/reference.py kv_quantize_fp4_ref is the torch statement of it). A cache row is
// the D values of one (sequence, position, kv head), cut into D / 32 blocks of 32 consecutive columns (OCP
// MX): e2m1 elements, one e8m0 scale per block. Per layer: k, v uint8 [B][cap][Hkv][D / 2], element 2i in
// the low nibble of byte i, element 2i + 1 in the high one; k_scale, v_scale uint8 [B][cap][Hkv][D / 32],
// byte = e + 127. Per block:
//   amax = max |x_i| (fp32; 16-bit inputs convert exactly)
//   amax == 0: e = 0, every nibble 0 (also for -0.0). Otherwise (m, k) = frexp(amax) and
//   e = clamp(k - 3 + (m > 0.75), -127, 127): the smallest e with amax * 2^-e <= 6 = 0.75 * 2^3, so nothing
//   saturates
//   nibble_i = sign(x_i) << 3 | code, code 0 .. 7 for the magnitudes {0, 0.5, 1, 1.5, 2, 3, 4, 6}: round to
//   nearest of |x_i| * 2^-e, ties to the even code (0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2,
//   3.5 -> 4, 5 -> 4)
//   dequantized value = value(nibble) * 2^e, exact in fp32 (one corner aside: a block whose maximum is the
//   largest bf16 has e = 126 and that maximum rounds up to 4 * 2^126 = 2^128)
// Rows with non-finite values are outside the contract: they store something and touch no other row.
//
//   kv_quantize_fp4  prefill: the k and v views [B][S][Hkv][D] of the fused QKV activation into cache rows
//                    0 .. S - 1
//   rope_append_fp4  rope_append_kernel (T tokens per sequence, its rows and overflow rule) with a quantizing
//                    store: q rotated in place (bit-equal), the k row rotated in fp32, rounded once to the
//                    model dtype and then quantized, the v row quantized from its 16-bit values
//   attn_decode_fp4  one workgroup per (sequence, kv head, chunk of 256 keys), every query head of the GQA
//                    group from one read of the chunk, fp32 partials into attn_decode's workspace, its
//                    combine kernel after it. A key at or beyond kv_len[b] is never loaded: neither its bytes
//                    nor its scales.
// The stores quantize in integer arithmetic: the seven rounding boundaries t * 2^e are built as fp32 bit
// patterns and compared with |x_i|'s bits, so no product is formed, nothing underflows and no denormal mode
// matters. One lane owns 8 columns (one 32-bit word of nibbles), the 4 aligned neighbouring lanes of a block
// share the amax by two shuffles; the loops step whole waves, so the shuffles are wave-uniform.
//
// Design of attn_decode_fp4. A 16-B load is exactly one MX block, so LPK = D / 32 lanes cover a row: at
// D = 128 a wave-load is 16 rows, four times the 16-bit kernel's. What grows with that is the cross-lane
// reduction of P.V, whose cost is per wave and not per byte: 64 / LPK lanes hold partial sums of the same
// columns. Two choices, made from instruction counts (neither has an A/B on the GPU), keep it below the FMA work:
//   * 4 waves per workgroup, not 8: a lane owns kKC4 / (4 * 64 / LPK) rows of K and of V (4 at D = 128),
//     all loaded, with their scale bytes, before the first use; more workgroups share a CU instead.
//   * the first three levels of the reduction are transposing: at each, a lane keeps half of its 8 columns
//     and sends the other half to its partner (4 + 2 + 1 shuffles instead of 8 + 8 + 8); the remaining
//     levels add one value. Every column's sum still has one fixed order.
// K side: the nibbles become 16-bit pairs of the unscaled e2m1 values through v_cvt_scalef32_pk_{bf16,f16}_fp4
// with scale 1 (exact), the packed dot accumulates a block's 32 products in fp32, and the block's 2^e
// multiplies that fp32 sum: no 16-bit value carries a scale. V side: the probability times the key's block
// scale (fp32, exact) is FMA'd onto the nibbles converted to fp32 (v_cvt_scalef32_pk_f32_fp4, scale 1), 8
// columns (one word) at a time so that 8 * GT accumulators are live.
// Measured on MI355X (profiles/decode/README.md, fp4 section; 16-bit / fp8 / fp4 in one process): 92.9 / 60.7 /
// 50.6 us at B 16, ctx 2048, MHA 32, D 128 and 18.1 / 16.7 / 14.0 us at B 1, ctx 8192, GQA 32/8. At 2.8 TB/s of
// the bytes it reads the kernel is bound by its instruction stream, not by HBM. Not built, not measured: 8
// waves per workgroup, two chunks per workgroup, a plain butterfly, the hardware convert in the stores.
#include "common.h"

#include <math.h>

extern "C" {
int pra_attn_decode_chunk();
hipError_t pra_attn_decode_combine(int dtype, const float* ws_o, const float* ws_ml, const int* kv_len, void* o,
                                   float* lse, int B, int Hq, int D, int cap, int NC, hipStream_t s);
}

namespace pra {

// Keys per chunk: the combine kernel of attention_decode.hip derives a sequence's chunk count from its own
// chunk length, so the two must be equal (the launcher checks).
constexpr int kKC4 = 256;
constexpr int kDec4Waves = 4;
constexpr int kDec4Threads = 64 * kDec4Waves;
constexpr float kDec4NoMax = -1e30f;  // as kDecNoMax

typedef __bf16 q4_bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 q4_f16x2 __attribute__((ext_vector_type(2)));
typedef float q4_f32x2 __attribute__((ext_vector_type(2)));

// ---- the rule, in integers ------------------------------------------------------------------------------
// the block's exponent from its amax (>= 0): frexp on the bits. A subnormal amax has k <= -126: below the clamp
__device__ __forceinline__ int fp4_scale_exp(float amax) {
  const uint32_t bits = __float_as_uint(amax) & 0x7fffffffu;
  if (bits == 0u) return 0;
  const int E = (int)(bits >> 23);
  // amax = 1.f * 2^(E - 127) = m * 2^k with k = E - 126; m > 0.75 <=> the fraction field > 0.5
  const int e = E - 129 + ((bits & 0x7fffffu) > 0x400000u ? 1 : 0);
  return min(max(e, -127), 127);
}
// bits of the fp32 value (mant24 * 2^-23) * 2^(field - 127), mant24 in [2^23, 2^24); field <= 0: subnormal. The
// callers' mantissas have two fraction bits and field >= -2, so the shift drops nothing.
__device__ __forceinline__ uint32_t fp4_bound(uint32_t mant24, int field) {
  return field >= 1 ? ((uint32_t)field << 23) | (mant24 & 0x7fffffu) : mant24 >> (1 - field);
}
// 8 values to 8 nibbles (element i in bits 4i .. 4i + 3) at block exponent e; amax is the block's
__device__ __forceinline__ uint32_t fp4_quant8(const float (&x)[8], int e, float amax) {
  if (amax == 0.f) return 0u;
  const int f = e + 127;
  // the boundaries between neighbouring codes, times 2^e; a tie belongs to the even code
  const uint32_t b1 = fp4_bound(0x800000u, f - 2);  // 0.25: above it code >= 1
  const uint32_t b2 = fp4_bound(0xc00000u, f - 1);  // 0.75: at or above it code >= 2
  const uint32_t b3 = fp4_bound(0xa00000u, f);      // 1.25: above
  const uint32_t b4 = fp4_bound(0xe00000u, f);      // 1.75: at or above
  const uint32_t b5 = fp4_bound(0xa00000u, f + 1);  // 2.5: above
  const uint32_t b6 = fp4_bound(0xe00000u, f + 1);  // 3.5: at or above
  const uint32_t b7 = fp4_bound(0xa00000u, f + 2);  // 5: above
  uint32_t w = 0u;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint32_t bits = __float_as_uint(x[i]);
    const uint32_t a = bits & 0x7fffffffu;
    const uint32_t code = (uint32_t)(a > b1) + (uint32_t)(a >= b2) + (uint32_t)(a > b3) + (uint32_t)(a >= b4) +
                          (uint32_t)(a > b5) + (uint32_t)(a >= b6) + (uint32_t)(a > b7);
    w |= ((bits >> 31) << 3 | code) << (4 * i);
  }
  return w;
}
// 2^(byte - 127) as fp32; byte 0 is the subnormal 2^-127
__device__ __forceinline__ float fp4_scale_of(uint32_t byte) {
  return __uint_as_float(byte != 0u ? byte << 23 : 0x00400000u);
}

__device__ __forceinline__ float fp4_amax8(const float (&x)[8]) {
  float a = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) a = fmaxf(a, fabsf(x[i]));
  return a;
}
// max over the 4 aligned neighbouring lanes of a block; every lane of the wave calls it
__device__ __forceinline__ float fp4_block_amax(float a) {
  a = fmaxf(a, __shfl_xor(a, 1, 64));
  return fmaxf(a, __shfl_xor(a, 2, 64));
}

// k, v [B * S][ld] views (Hkv * D columns each); one lane per 8 columns, k rows first, then v rows.
template <typename T>
__global__ __launch_bounds__(256) void kv_quantize_fp4_kernel(const T* __restrict__ k, const T* __restrict__ v,
                                                              uint8_t* __restrict__ kq, uint8_t* __restrict__ vq,
                                                              uint8_t* __restrict__ ks, uint8_t* __restrict__ vs, int B,
                                                              int S, long ld, int Hkv, int D, int cap) {
  const int vpt = Hkv * D / 8;  // 8-column vectors per token of one tensor (a multiple of 4: whole blocks)
  const long per = (long)B * S * vpt;
  const long total = 2 * per;
  const int lane = threadIdx.x & 63;
  for (long base = (long)blockIdx.x * 256 + (threadIdx.x - lane); base < total; base += (long)gridDim.x * 256) {
    const long idx = base + lane;
    const bool live = idx < total;  // a block's 4 lanes are all live or all not
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
    const float amax = fp4_block_amax(fp4_amax8(x));
    const int e = fp4_scale_exp(amax);
    if (live) {
      const long b = tok / S;
      const long row = b * cap + (tok - b * S);
      // 4 bytes of the row's Hkv * D / 2; the 4 lanes of a block write its 16 bytes
      *reinterpret_cast<uint32_t*>((isv ? vq : kq) + row * (vpt * 4) + c * 4) = fp4_quant8(x, e, amax);
      if ((c & 3) == 0) (isv ? vs : ks)[row * (vpt / 4) + c / 4] = (uint8_t)(e + 127);
    }
  }
}

// (a + ib) * (c + is): rope_append_kernel's dec_rot_pair, which is elementwise.hip's rot_pair
__device__ __forceinline__ void q4_rot_pair(float a, float b, float c, float s, float& o0, float& o1) {
  o0 = __builtin_fmaf(a, c, -(b * s));
  o1 = __builtin_fmaf(a, s, b * c);
}

// qkv [B * nt][ld]: q (Hq heads) | k (Hkv) | v (Hkv), D columns each, row b * nt + t at position
// clamp(kv_len[b], 0, cap) + t. One lane per 8 columns. nt == 1 clamps the row to cap - 1; with nt > 1 a
// position at or beyond cap stores nothing (its q takes table row cap - 1) but still takes part in the shuffles.
template <typename T>
__global__ __launch_bounds__(256) void rope_append_fp4_kernel(T* __restrict__ qkv, const float2* __restrict__ tab,
                                                              const int* __restrict__ kv_len, uint8_t* __restrict__ kq,
                                                              uint8_t* __restrict__ vq, uint8_t* __restrict__ ks,
                                                              uint8_t* __restrict__ vs, int B, int nt, long ld, int Hq,
                                                              int Hkv, int D, int cap) {
  const int nq = Hq * D, nk = Hkv * D;
  const int vpr = (nq + 2 * nk) / 8;  // a multiple of 4
  const long total = (long)B * nt * vpr;
  const int lane = threadIdx.x & 63;
  for (long base = (long)blockIdx.x * 256 + (threadIdx.x - lane); base < total; base += (long)gridDim.x * 256) {
    const long idx = base + lane;
    const bool live = idx < total;
    float x[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};  // what this lane quantizes (k, v lanes)
    int kind = 0;                                            // 1: k row, 2: v row (0 also for a row that is not stored)
    long row = 0;
    int cin = 0;  // column inside the k (or v) part
    if (live) {
      const long r = idx / vpr;  // row b * nt + t
      const int b = (int)(r / nt);
      const int col = (int)(idx - r * vpr) * 8;
      const int at = min(max(kv_len[b], 0), cap) + (int)(r - (long)b * nt);  // <= cap + nt - 1
      const int pos = min(at, cap - 1);
      const bool keep = at < cap || nt == 1;  // one token: the clamped row is overwritten
      T* p = qkv + r * ld + col;
      float v[8];
      load8<T>(p, v);
      row = (long)b * cap + pos;
      if (col >= nq + nk) {
        kind = keep ? 2 : 0;
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
        for (int j = 0; j < 4; ++j) q4_rot_pair(v[2 * j], v[2 * j + 1], c[j], s[j], o[2 * j], o[2 * j + 1]);
        if (col < nq) {
          store8<T>(p, o);
        } else {
          kind = keep ? 1 : 0;
          cin = col - nq;
#pragma unroll
          for (int i = 0; i < 8; ++i) x[i] = rnd<T>(o[i]);  // what the 16-bit cache would hold
        }
      }
    }
    const float amax = fp4_block_amax(fp4_amax8(x));
    const int e = fp4_scale_exp(amax);
    if (kind != 0) {
      *reinterpret_cast<uint32_t*>((kind == 2 ? vq : kq) + row * (nk / 2) + cin / 2) = fp4_quant8(x, e, amax);
      if (cin % 32 == 0) (kind == 2 ? vs : ks)[row * (nk / 32) + cin / 32] = (uint8_t)(e + 127);
    }
  }
}

// ---- decode -----------------------------------------------------------------------------------------------
// 8 columns of q (one 16-B load of 16-bit pairs) against one word of 8 nibbles: the nibbles become 16-bit
// pairs of the unscaled e2m1 values (exact; scale operand 1), four packed dots with fp32 accumulate.
template <typename T>
__device__ __forceinline__ float dot8_fp4(const uint4& q, uint32_t kw, float c);
template <>
__device__ __forceinline__ float dot8_fp4<__bf16>(const uint4& q, uint32_t kw, float c) {
  c = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(q4_bf16x2, q.x), __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(kw, 1.0f, 0), c, false);
  c = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(q4_bf16x2, q.y), __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(kw, 1.0f, 1), c, false);
  c = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(q4_bf16x2, q.z), __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(kw, 1.0f, 2), c, false);
  c = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(q4_bf16x2, q.w), __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(kw, 1.0f, 3), c, false);
  return c;
}
template <>
__device__ __forceinline__ float dot8_fp4<__half>(const uint4& q, uint32_t kw, float c) {
  c = __builtin_amdgcn_fdot2(__builtin_bit_cast(q4_f16x2, q.x), __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(kw, 1.0f, 0), c, false);
  c = __builtin_amdgcn_fdot2(__builtin_bit_cast(q4_f16x2, q.y), __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(kw, 1.0f, 1), c, false);
  c = __builtin_amdgcn_fdot2(__builtin_bit_cast(q4_f16x2, q.z), __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(kw, 1.0f, 2), c, false);
  c = __builtin_amdgcn_fdot2(__builtin_bit_cast(q4_f16x2, q.w), __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(kw, 1.0f, 3), c, false);
  return c;
}

// one word of 8 nibbles as fp32 (exact); zeros for a key that was never loaded
__device__ __forceinline__ void unpack8_fp4(uint32_t w, float (&o)[8]) {
  const q4_f32x2 a = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, 1.0f, 0);
  const q4_f32x2 b = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, 1.0f, 1);
  const q4_f32x2 c = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, 1.0f, 2);
  const q4_f32x2 d = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, 1.0f, 3);
  o[0] = a.x, o[1] = a.y, o[2] = b.x, o[3] = b.y, o[4] = c.x, o[5] = c.y, o[6] = d.x, o[7] = d.y;
}

// Partials as attn_decode_chunk_kernel: ws_o [B][Hq][NC][D] fp32 (unnormalised), ws_ml [B][Hq][NC][2].
// grid (NC, Hkv * (G / GT), B). LPK = D / 32 lanes cover one cache row (16 B, one MX block, each), a wave-load
// covers KPW = 64 / LPK rows, the workgroup's 4 waves KPB = 4 * KPW consecutive rows per step. lane = ks * LPK +
// part: part is the block of the row, ks the row of the wave-load.
template <typename T, int D, int GT>
__global__ __launch_bounds__(kDec4Threads) void attn_decode_fp4_chunk_kernel(
    const T* __restrict__ q, const uint8_t* __restrict__ kc, const uint8_t* __restrict__ vc,
    const uint8_t* __restrict__ ksc, const uint8_t* __restrict__ vsc, const int* __restrict__ kv_len,
    float* __restrict__ ws_o, float* __restrict__ ws_ml, int Hq, int Hkv, int cap, int NC, float scale_log2) {
  constexpr int LPK = D / 32;
  constexpr int KPW = 64 / LPK;
  constexpr int KPB = kDec4Waves * KPW;
  constexpr int STEPS = kKC4 / KPB;  // rows of K (and of V) per lane
  static_assert(kKC4 % KPB == 0 && STEPS >= 1 && KPW >= 8, "chunk must tile; three transposing levels");
  __shared__ float s_p[kKC4 * GT];              // [key][g]: scores, then probabilities
  __shared__ float s_red[kDec4Waves * GT * D];  // [wave][g][d]: per-wave P.V

  const int b = blockIdx.z;
  const int G = Hq / Hkv;
  const int tiles = G / GT;
  const int hkv = blockIdx.y / tiles;
  const int h0 = hkv * G + (blockIdx.y - hkv * tiles) * GT;  // first query head served here
  const int chunk = blockIdx.x;
  const int len = min(max(kv_len[b], 0), cap);
  const int c0 = chunk * kKC4;
  if (c0 >= len) return;  // wave-uniform: nothing read, nothing written

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int part = lane % LPK;  // which block (32 columns) of the row
  const int ks = lane / LPK;    // which row of the wave-load
  const long tok_stride = (long)Hkv * (D / 2);  // bytes
  const long tok_scales = (long)Hkv * LPK;
  const long data0 = ((long)b * cap + c0) * tok_stride + (long)hkv * (D / 2) + part * 16;
  const long scale0 = ((long)b * cap + c0) * tok_scales + (long)hkv * LPK + part;

  // every load of the chunk, K first; a key at or beyond len is never loaded (zeros stand in)
  uint4 kraw[STEPS], vraw[STEPS];
  uint32_t ke[STEPS], ve[STEPS];
#pragma unroll
  for (int st = 0; st < STEPS; ++st) {
    const int kl = st * KPB + wave * KPW + ks;  // key within the chunk
    kraw[st] = make_uint4(0u, 0u, 0u, 0u);
    ke[st] = 127u;
    if (c0 + kl < len) {
      kraw[st] = *reinterpret_cast<const uint4*>(kc + data0 + (long)kl * tok_stride);
      ke[st] = ksc[scale0 + (long)kl * tok_scales];
    }
  }
#pragma unroll
  for (int st = 0; st < STEPS; ++st) {
    const int kl = st * KPB + wave * KPW + ks;
    vraw[st] = make_uint4(0u, 0u, 0u, 0u);
    ve[st] = 127u;
    if (c0 + kl < len) {
      vraw[st] = *reinterpret_cast<const uint4*>(vc + data0 + (long)kl * tok_stride);
      ve[st] = vsc[scale0 + (long)kl * tok_scales];
    }
  }

  // ---- phase 1: scores ---------------------------------------------------------------
  {
    uint4 qv[GT][4];  // the lane's 32 columns of every head
#pragma unroll
    for (int g = 0; g < GT; ++g) {
      const uint4* qp = reinterpret_cast<const uint4*>(q + ((long)b * Hq + h0 + g) * D + part * 32);
#pragma unroll
      for (int j = 0; j < 4; ++j) qv[g][j] = qp[j];
    }
#pragma unroll
    for (int st = 0; st < STEPS; ++st) {
      const int kl = st * KPB + wave * KPW + ks;
      const uint32_t kw[4] = {kraw[st].x, kraw[st].y, kraw[st].z, kraw[st].w};
      const float f = fp4_scale_of(ke[st]);
      float d[GT];
#pragma unroll
      for (int g = 0; g < GT; ++g) {
        float c = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) c = dot8_fp4<T>(qv[g][j], kw[j], c);
        d[g] = c * f;  // the block's 2^e on the fp32 block sum
      }
#pragma unroll
      for (int o = 1; o < LPK; o <<= 1) {
#pragma unroll
        for (int g = 0; g < GT; ++g) d[g] += __shfl_xor(d[g], o, 64);
      }
      if (part == 0) {
        const bool valid = c0 + kl < len;
#pragma unroll
        for (int g = 0; g < GT; ++g) s_p[kl * GT + g] = valid ? d[g] * scale_log2 : -INFINITY;
      }
    }
  }
  __syncthreads();

  // ---- phase 2: per head, exact max, probabilities, their sum (one wave per head)
  for (int g = wave; g < GT; g += kDec4Waves) {
    float sv[kKC4 / 64];
    float m = kDec4NoMax;
#pragma unroll
    for (int i = 0; i < kKC4 / 64; ++i) {
      sv[i] = s_p[(i * 64 + lane) * GT + g];
      m = fmaxf(m, sv[i]);
    }
    m = wave_max(m);
    float l = 0.f;
#pragma unroll
    for (int i = 0; i < kKC4 / 64; ++i) {
      const float p = exp2f(sv[i] - m);  // masked key: exp2(-inf) = 0, m is finite
      s_p[(i * 64 + lane) * GT + g] = p;
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

  // ---- phase 3: P.V, one word (8 of the lane's 32 columns) at a time -----------------------------------
  float vf32[STEPS];  // the V block scales; 1 for a masked key, whose p and nibbles are 0
#pragma unroll
  for (int st = 0; st < STEPS; ++st) vf32[st] = fp4_scale_of(ve[st]);
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    float acc[GT][8];
#pragma unroll
    for (int g = 0; g < GT; ++g)
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[g][i] = 0.f;
#pragma unroll
    for (int st = 0; st < STEPS; ++st) {
      const int kl = st * KPB + wave * KPW + ks;
      const uint32_t vw = w == 0 ? vraw[st].x : w == 1 ? vraw[st].y : w == 2 ? vraw[st].z : vraw[st].w;
      float vf[8];
      unpack8_fp4(vw, vf);
#pragma unroll
      for (int g = 0; g < GT; ++g) {
        const float p = s_p[kl * GT + g] * vf32[st];  // exact: a power of two
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[g][i] = __builtin_fmaf(p, vf[i], acc[g][i]);
      }
    }
    // Over the KPW rows of the wave-load (lanes with the same `part`). Levels 0 .. 2 transpose: the lane whose
    // ks bit j is 0 keeps the lower half of its columns and receives the partner's lower half, the other lane
    // the upper halves; afterwards acc[g][0] holds column ((ks & 1) << 2) | (ks & 2) | ((ks >> 2) & 1).
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int o = LPK << j, h = 4 >> j;
      const bool up = (lane & o) != 0;
#pragma unroll
      for (int g = 0; g < GT; ++g)
#pragma unroll
        for (int i = 0; i < h; ++i) {
          const float keep = up ? acc[g][i + h] : acc[g][i];
          const float send = up ? acc[g][i] : acc[g][i + h];
          acc[g][i] = keep + __shfl_xor(send, o, 64);
        }
    }
#pragma unroll
    for (int o = LPK << 3; o < 64; o <<= 1) {
#pragma unroll
      for (int g = 0; g < GT; ++g) acc[g][0] += __shfl_xor(acc[g][0], o, 64);
    }
    if (ks < 8) {
      const int col = part * 32 + w * 8 + (((ks & 1) << 2) | (ks & 2) | ((ks >> 2) & 1));
#pragma unroll
      for (int g = 0; g < GT; ++g) s_red[(wave * GT + g) * D + col] = acc[g][0];
    }
  }
  __syncthreads();
  // the waves in order
  for (int e = tid; e < GT * D; e += kDec4Threads) {
    const int g = e / D, dcol = e - g * D;
    float s = s_red[e];
#pragma unroll
    for (int w = 1; w < kDec4Waves; ++w) s += s_red[w * GT * D + e];
    ws_o[(((long)b * Hq + h0 + g) * NC + chunk) * D + dcol] = s;
  }
}

template <typename T, int D, int GT>
static hipError_t launch_chunks_fp4(const void* q, const void* kc, const void* vc, const void* ksc, const void* vsc,
                                    const int* kv_len, float* ws_o, float* ws_ml, int B, int Hq, int Hkv, int cap,
                                    int NC, float scale, hipStream_t st) {
  const int tiles = (Hq / Hkv) / GT;
  hipLaunchKernelGGL((attn_decode_fp4_chunk_kernel<T, D, GT>), dim3(NC, Hkv * tiles, B), dim3(kDec4Threads), 0, st,
                     (const T*)q, (const uint8_t*)kc, (const uint8_t*)vc, (const uint8_t*)ksc, (const uint8_t*)vsc,
                     kv_len, ws_o, ws_ml, Hq, Hkv, cap, NC, scale * 1.4426950408889634f);
  return hipGetLastError();
}

template <typename T, int D>
static hipError_t launch_decode_fp4(const void* q, const void* kc, const void* vc, const void* ksc, const void* vsc,
                                    const int* kv_len, float* ws_o, float* ws_ml, int B, int Hq, int Hkv, int cap,
                                    int NC, float scale, hipStream_t st) {
  const int G = Hq / Hkv;
  // the widest head tile that divides the group, as the 16-bit kernel
  if (G % 8 == 0) return launch_chunks_fp4<T, D, 8>(q, kc, vc, ksc, vsc, kv_len, ws_o, ws_ml, B, Hq, Hkv, cap, NC, scale, st);
  if (G % 4 == 0) return launch_chunks_fp4<T, D, 4>(q, kc, vc, ksc, vsc, kv_len, ws_o, ws_ml, B, Hq, Hkv, cap, NC, scale, st);
  if (G % 2 == 0) return launch_chunks_fp4<T, D, 2>(q, kc, vc, ksc, vsc, kv_len, ws_o, ws_ml, B, Hq, Hkv, cap, NC, scale, st);
  return launch_chunks_fp4<T, D, 1>(q, kc, vc, ksc, vsc, kv_len, ws_o, ws_ml, B, Hq, Hkv, cap, NC, scale, st);
}

}  // namespace pra

extern "C" {

int pra_attn_decode_fp4_chunk() { return pra::kKC4; }

hipError_t pra_kv_quantize_fp4(int dtype, const void* k, const void* v, long ld, void* k_cache, void* v_cache,
                               void* k_scale, void* v_scale, int B, int S, int Hkv, int D, int cap, hipStream_t s) {
  if (B <= 0 || S <= 0 || S > cap || Hkv <= 0 || (D != 64 && D != 128) || ld % 8 || ld < (long)Hkv * D)
    return hipErrorInvalidValue;
  const long items = 2L * B * S * Hkv * D / 8;
  long grid = (items + 255) / 256;
  if (grid > 4096) grid = 4096;
  PRA_DISPATCH_16BIT(dtype, T,
                     hipLaunchKernelGGL((pra::kv_quantize_fp4_kernel<T>), dim3((unsigned)grid), dim3(256), 0, s,
                                        (const T*)k, (const T*)v, (uint8_t*)k_cache, (uint8_t*)v_cache,
                                        (uint8_t*)k_scale, (uint8_t*)v_scale, B, S, ld, Hkv, D, cap));
  return hipGetLastError();
}

hipError_t pra_rope_append_fp4(int dtype, void* qkv, const void* tab, const int* kv_len, void* k_cache, void* v_cache,
                               void* k_scale, void* v_scale, int B, int nt, long ld, int Hq, int Hkv, int D, int cap,
                               hipStream_t s) {
  if (B <= 0 || nt <= 0 || cap <= 0 || Hq <= 0 || Hkv <= 0 || (D != 64 && D != 128) || ld % 8)
    return hipErrorInvalidValue;
  const long items = (long)B * nt * (Hq + 2 * Hkv) * D / 8;
  long grid = (items + 255) / 256;
  if (grid > 2048) grid = 2048;
  PRA_DISPATCH_16BIT(dtype, T,
                     hipLaunchKernelGGL((pra::rope_append_fp4_kernel<T>), dim3((unsigned)grid), dim3(256), 0, s,
                                        (T*)qkv, (const float2*)tab, kv_len, (uint8_t*)k_cache, (uint8_t*)v_cache,
                                        (uint8_t*)k_scale, (uint8_t*)v_scale, B, nt, ld, Hq, Hkv, D, cap));
  return hipGetLastError();
}

hipError_t pra_attn_decode_fp4(int dtype, const void* q, const void* k_cache, const void* v_cache, const void* k_scale,
                               const void* v_scale, const int* kv_len, void* o, float* lse, float* ws, int B, int Hq,
                               int Hkv, int D, int cap, float scale, hipStream_t s) {
  if (B <= 0 || cap <= 0 || Hkv <= 0 || Hq % Hkv || B > 65535 || Hq > 65535) return hipErrorInvalidValue;
  if (pra_attn_decode_chunk() != pra::kKC4) return hipErrorInvalidValue;  // the shared combine kernel's chunking
  const int NC = (cap + pra::kKC4 - 1) / pra::kKC4;
  float* ws_o = ws;
  float* ws_ml = ws + (long)B * Hq * NC * D;
  hipError_t e = hipErrorInvalidValue;
  PRA_DISPATCH_16BIT(dtype, T, {
    if (D == 64)
      e = pra::launch_decode_fp4<T, 64>(q, k_cache, v_cache, k_scale, v_scale, kv_len, ws_o, ws_ml, B, Hq, Hkv, cap, NC, scale, s);
    else if (D == 128)
      e = pra::launch_decode_fp4<T, 128>(q, k_cache, v_cache, k_scale, v_scale, kv_len, ws_o, ws_ml, B, Hq, Hkv, cap, NC, scale, s);
  });
  if (e != hipSuccess) return e;
  return pra_attn_decode_combine(dtype, ws_o, ws_ml, kv_len, o, lse, B, Hq, D, cap, NC, s);
}
}
