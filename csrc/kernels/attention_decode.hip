// KV-cache generation: the two kernels of a decode step (bf16 / fp16, head_dim 64 / 128).
//
// Cache layout, per layer: k_cache, v_cache [B][cap][Hkv][D], token-major like every other activation
// here. kv_len is int32 [B] ON THE DEVICE: no launch argument depends on a host copy of it, so a decode
// step never synchronises.
//
//   rope_append  the fused QKV rows of T new tokens per sequence (row b * T + t at position
//                p = kv_len[b] + t): q rotated in place, rotated k and plain v written into cache row p.
//                The rotation is rope_kernel's (elementwise.hip): same table, rot_pair in fp32, one
//                rounding -- bit-equal to it. T = 1 (a decode step) clamps the row into the cache:
//                pos[b] = clamp(kv_len[b], 0, cap - 1). With T > 1 (attention_extend.hip) a row with
//                p >= cap stores nothing and its q is rotated with table row cap - 1.
//   attn_decode  one query per sequence over keys 0 .. kv_len[b] - 1. The kernel streams K and V once
//                (about Hq/Hkv flop per byte: the target is bytes per second), so the cache rows go
//                straight to VGPRs as 16-B loads, all of a chunk's in flight at once, and the dot
//                products run on the VALU (packed 16-bit dot with fp32 accumulate for q.k, fp32 FMA for p.v).
//
// Decomposition of attn_decode. Keys are cut into chunks of a FIXED length kKC; chunk boundaries are a
// function of the key position only. One workgroup owns one (sequence, kv head, chunk) and serves
// every query head of the GQA group from one read of K and V. Inside a chunk: scores of all kKC keys
// into LDS, an exact max and the probabilities per head, then P.V. The chunk's fp32 partial
// (max, sum, o) goes to a workspace and a second kernel merges the partials of a (sequence, head) in
// ascending chunk order. No float atomics, no workgroup waits for another, and every sum has one
// fixed order, so (a) two runs give the same bits and (b) a sequence's output is a function of its
// own q, K, V and length alone: not of the batch, the other lengths or cap.
// Chunks at or beyond kv_len[b] leave at once without touching the cache, and inside the last
// chunk keys at or beyond kv_len[b] are never loaded: whatever the cache holds there (NaN, Inf) cannot
// reach the output. The running max starts at a finite sentinel (as attention_docs.hip), so length 0
// gives o = 0, lse = -inf without a NaN.
#include "common.h"

#include <math.h>

namespace pra {

// Keys per chunk, chosen by measurement on MI355X (tools/decode_bench.py; profiles/decode/README.md: 256
// beats 128 and 512 at both shapes measured).
constexpr int kKC = 256;
static_assert(kKC % 64 == 0 && kKC >= 64, "chunk length");
constexpr int kDecWaves = 8;
constexpr int kDecThreads = 64 * kDecWaves;
constexpr float kDecNoMax = -1e30f;    // "no score yet" (log2 units; real scores are far above)

// (a + ib) * (c + is): the FMA placement of elementwise.hip's rot_pair, which rope_append must match bit for bit
__device__ __forceinline__ void dec_rot_pair(float a, float b, float c, float s, float& o0, float& o1) {
  o0 = __builtin_fmaf(a, c, -(b * s));
  o1 = __builtin_fmaf(a, s, b * c);
}

// qkv [B * nt][ld]: q (Hq heads) | k (Hkv) | v (Hkv), D columns each. One lane per 8 columns.
template <typename T>
__global__ __launch_bounds__(256) void rope_append_kernel(T* __restrict__ qkv, const float2* __restrict__ tab,
                                                          const int* __restrict__ kv_len, T* __restrict__ kc,
                                                          T* __restrict__ vc, int B, int nt, long ld, int Hq, int Hkv,
                                                          int D, int cap) {
  const int nq = Hq * D, nk = Hkv * D;
  const int vpr = (nq + 2 * nk) / 8;
  const long total = (long)B * nt * vpr;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const long r = idx / vpr;  // row b * nt + t
    const int b = (int)(r / nt);
    const int col = (int)(idx - r * vpr) * 8;
    const int at = min(max(kv_len[b], 0), cap) + (int)(r - (long)b * nt);  // <= cap + nt - 1
    const int pos = min(at, cap - 1);
    const bool keep = at < cap || nt == 1;  // one token: the clamped row is overwritten
    T* p = qkv + r * ld + col;
    float v[8];
    load8<T>(p, v);
    const long row = ((long)b * cap + pos) * nk;  // cache row of this token, in elements
    if (col >= nq + nk) {
      if (keep) store8<T>(vc + row + (col - nq - nk), v);  // exact copy
      continue;
    }
    const int pi = (col % D) / 2;
    const float4* tp = reinterpret_cast<const float4*>(tab + (size_t)pos * (D / 2) + pi);
    const float4 cs01 = tp[0], cs23 = tp[1];
    const float c[4] = {cs01.x, cs01.z, cs23.x, cs23.z};
    const float s[4] = {cs01.y, cs01.w, cs23.y, cs23.w};
    float o[8];
#pragma unroll
    for (int k = 0; k < 4; ++k) dec_rot_pair(v[2 * k], v[2 * k + 1], c[k], s[k], o[2 * k], o[2 * k + 1]);
    if (col < nq)
      store8<T>(p, o);
    else if (keep)
      store8<T>(kc + row + (col - nq), o);
  }
}

// 8 stored elements of a cache row as raw bits (zero where the key is masked: never loaded)
template <typename T>
__device__ __forceinline__ void unpack8(const uint4& raw, float (&o)[8]);
template <>
__device__ __forceinline__ void unpack8<__bf16>(const uint4& raw, float (&o)[8]) {
  const uint32_t w[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    o[2 * i] = __uint_as_float(w[i] << 16);
    o[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
  }
}
template <>
__device__ __forceinline__ void unpack8<__half>(const uint4& raw, float (&o)[8]) {
  const __half* h = reinterpret_cast<const __half*>(&raw);
#pragma unroll
  for (int i = 0; i < 8; ++i) o[i] = __half2float(h[i]);
}

// 8-element dot product of two packed rows on the packed-dot VALU instruction (v_dot2c_f32_bf16 / _f16:
// fp32 accumulate, two products per instruction), straight from the loaded bits: no unpacking of K.
typedef __bf16 dec_bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 dec_f16x2 __attribute__((ext_vector_type(2)));
template <typename T>
__device__ __forceinline__ float dot8(const uint4& a, const uint4& b);
template <>
__device__ __forceinline__ float dot8<__bf16>(const uint4& a, const uint4& b) {
  float c = 0.f;
  c = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(dec_bf16x2, a.x), __builtin_bit_cast(dec_bf16x2, b.x), c, false);
  c = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(dec_bf16x2, a.y), __builtin_bit_cast(dec_bf16x2, b.y), c, false);
  c = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(dec_bf16x2, a.z), __builtin_bit_cast(dec_bf16x2, b.z), c, false);
  c = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(dec_bf16x2, a.w), __builtin_bit_cast(dec_bf16x2, b.w), c, false);
  return c;
}
template <>
__device__ __forceinline__ float dot8<__half>(const uint4& a, const uint4& b) {
  float c = 0.f;
  c = __builtin_amdgcn_fdot2(__builtin_bit_cast(dec_f16x2, a.x), __builtin_bit_cast(dec_f16x2, b.x), c, false);
  c = __builtin_amdgcn_fdot2(__builtin_bit_cast(dec_f16x2, a.y), __builtin_bit_cast(dec_f16x2, b.y), c, false);
  c = __builtin_amdgcn_fdot2(__builtin_bit_cast(dec_f16x2, a.z), __builtin_bit_cast(dec_f16x2, b.z), c, false);
  c = __builtin_amdgcn_fdot2(__builtin_bit_cast(dec_f16x2, a.w), __builtin_bit_cast(dec_f16x2, b.w), c, false);
  return c;
}

// Partials: ws_o [B][Hq][NC][D] fp32 (unnormalised), ws_ml [B][Hq][NC][2] = (max in log2 units, sum).
// grid (NC, Hkv * (G / GT), B); GT query heads of one kv head per workgroup.
// Lane layout: LPK = D / 8 lanes cover one cache row (16 B each), a wave-load covers 64 / LPK rows,
// the workgroup's 8 waves cover KPB = 8 * 64 / LPK consecutive rows per step. A lane issues the loads of
// all its K and V rows of the chunk (kKC / KPB each) before the first use: with one workgroup per CU (batch 1)
// the chunk's whole 2 * kKC rows are in flight at once, and V arrives under the score phase.
template <typename T, int D, int GT>
__global__ __launch_bounds__(kDecThreads) void attn_decode_chunk_kernel(
    const T* __restrict__ q, const T* __restrict__ kc, const T* __restrict__ vc, const int* __restrict__ kv_len,
    float* __restrict__ ws_o, float* __restrict__ ws_ml, int Hq, int Hkv, int cap, int NC, float scale_log2) {
  constexpr int LPK = D / 8;
  constexpr int KPW = 64 / LPK;
  constexpr int KPB = kDecWaves * KPW;
  constexpr int STEPS = kKC / KPB;  // rows of K (and of V) per lane
  static_assert(kKC % KPB == 0 && STEPS >= 1, "chunk must tile");
  __shared__ float s_p[kKC * GT];             // [key][g]: scores, then probabilities
  __shared__ float s_red[kDecWaves * GT * D]; // [wave][g][d]: per-wave P.V

  const int b = blockIdx.z;
  const int G = Hq / Hkv;
  const int tiles = G / GT;
  const int hkv = blockIdx.y / tiles;
  const int h0 = hkv * G + (blockIdx.y - hkv * tiles) * GT;  // first query head served here
  const int chunk = blockIdx.x;
  const int len = min(max(kv_len[b], 0), cap);
  const int c0 = chunk * kKC;
  if (c0 >= len) return;  // wave-uniform: nothing read, nothing written

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int part = lane % LPK;  // which 8 columns of the row
  const int ks = lane / LPK;    // which row of the wave-load
  const long tok_stride = (long)Hkv * D;
  const T* kbase = kc + ((long)b * cap + c0) * tok_stride + (long)hkv * D + part * 8;
  const T* vbase = vc + ((long)b * cap + c0) * tok_stride + (long)hkv * D + part * 8;

  // every load of the chunk, K first; a key at or beyond len is never loaded (zeros stand in)
  uint4 kraw[STEPS], vraw[STEPS];
#pragma unroll
  for (int st = 0; st < STEPS; ++st) {
    const int kl = st * KPB + wave * KPW + ks;  // key within the chunk
    kraw[st] = make_uint4(0u, 0u, 0u, 0u);
    if (c0 + kl < len) kraw[st] = *reinterpret_cast<const uint4*>(kbase + (long)kl * tok_stride);
  }
#pragma unroll
  for (int st = 0; st < STEPS; ++st) {
    const int kl = st * KPB + wave * KPW + ks;
    vraw[st] = make_uint4(0u, 0u, 0u, 0u);
    if (c0 + kl < len) vraw[st] = *reinterpret_cast<const uint4*>(vbase + (long)kl * tok_stride);
  }

  // ---- phase 1: scores ---------------------------------------------------------------
  {
    uint4 qraw[GT];
#pragma unroll
    for (int g = 0; g < GT; ++g) qraw[g] = *reinterpret_cast<const uint4*>(q + ((long)b * Hq + h0 + g) * D + part * 8);
    {
#pragma unroll
      for (int st = 0; st < STEPS; ++st) {
        const int kl = st * KPB + wave * KPW + ks;
        float d[GT];
#pragma unroll
        for (int g = 0; g < GT; ++g) d[g] = dot8<T>(qraw[g], kraw[st]);
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
  }
  __syncthreads();

  // ---- phase 2: per head, exact max, probabilities, their sum (one wave per head)
  for (int g = wave; g < GT; g += kDecWaves) {
    float sv[kKC / 64];
    float m = kDecNoMax;
#pragma unroll
    for (int i = 0; i < kKC / 64; ++i) {
      sv[i] = s_p[(i * 64 + lane) * GT + g];
      m = fmaxf(m, sv[i]);
    }
    m = wave_max(m);
    float l = 0.f;
#pragma unroll
    for (int i = 0; i < kKC / 64; ++i) {
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

  // ---- phase 3: P.V --------------------------------------------------------------------
  float acc[GT][8];
#pragma unroll
  for (int g = 0; g < GT; ++g)
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[g][i] = 0.f;
  {
#pragma unroll
    for (int st = 0; st < STEPS; ++st) {
      const int kl = st * KPB + wave * KPW + ks;
      float vf[8];
      unpack8<T>(vraw[st], vf);  // zeros for a masked key, whose p is 0 too
#pragma unroll
      for (int g = 0; g < GT; ++g) {
        const float p = s_p[kl * GT + g];
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[g][i] = __builtin_fmaf(p, vf[i], acc[g][i]);
      }
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
      for (int i = 0; i < 8; ++i) s_red[(wave * GT + g) * D + part * 8 + i] = acc[g][i];
  }
  __syncthreads();
  for (int e = tid; e < GT * D; e += kDecThreads) {
    const int g = e / D, dcol = e - g * D;
    float s = s_red[e];
#pragma unroll
    for (int w = 1; w < kDecWaves; ++w) s += s_red[w * GT * D + e];
    ws_o[(((long)b * Hq + h0 + g) * NC + chunk) * D + dcol] = s;
  }
}

// grid (Hq, B), D threads: merges the chunk partials of one (sequence, head) in ascending chunk order.
// The chunks' weights exp2(m_c - M) are formed 64 at a time by the first wave (independent loads) and
// shared through LDS; every lane then adds its column of the 64 partials in order, the loads of eight
// chunks in flight together (nothing in the loop waits on the previous chunk's load).
template <typename T, int D>
__global__ __launch_bounds__(D) void attn_decode_combine_kernel(const float* __restrict__ ws_o,
                                                                const float* __restrict__ ws_ml,
                                                                const int* __restrict__ kv_len, T* __restrict__ o,
                                                                float* __restrict__ lse, int Hq, int cap, int NC) {
  __shared__ float s_w[64], s_l[64], s_scr[D / 64];
  const int h = blockIdx.x, b = blockIdx.y, d = threadIdx.x;
  const int len = min(max(kv_len[b], 0), cap);
  const int nc = (len + kKC - 1) / kKC;  // <= NC
  const long bh = (long)b * Hq + h;
  const float* ml = ws_ml + bh * NC * 2;
  const float* po = ws_o + bh * NC * D + d;
  float M = kDecNoMax;
  for (int c = d; c < nc; c += D) M = fmaxf(M, ml[2 * c]);
  M = block_max<D / 64>(M, s_scr);  // >= the sentinel: finite
  float L = 0.f, O = 0.f;
  for (int c0 = 0; c0 < nc; c0 += 64) {
    const int n = min(64, nc - c0);
    if (d < n) {
      s_w[d] = exp2f(ml[2 * (c0 + d)] - M);
      s_l[d] = ml[2 * (c0 + d) + 1];
    }
    __syncthreads();
#pragma unroll 8
    for (int j = 0; j < n; ++j) {
      const float w = s_w[j];
      L = __builtin_fmaf(s_l[j], w, L);
      O = __builtin_fmaf(po[(long)(c0 + j) * D], w, O);
    }
    __syncthreads();
  }
  o[bh * D + d] = from_f<T>(nc > 0 ? O / L : 0.f);
  if (d == 0) lse[bh] = nc > 0 ? (M + log2f(L)) * 0.6931471805599453f : -INFINITY;
}

template <typename T, int D, int GT>
static hipError_t launch_chunks(const void* q, const void* kc, const void* vc, const int* kv_len, float* ws_o,
                                float* ws_ml, int B, int Hq, int Hkv, int cap, int NC, float scale, hipStream_t st) {
  const int tiles = (Hq / Hkv) / GT;
  hipLaunchKernelGGL((attn_decode_chunk_kernel<T, D, GT>), dim3(NC, Hkv * tiles, B), dim3(kDecThreads), 0, st,
                     (const T*)q, (const T*)kc, (const T*)vc, kv_len, ws_o, ws_ml, Hq, Hkv, cap, NC,
                     scale * 1.4426950408889634f);
  return hipGetLastError();
}

template <typename T, int D>
static hipError_t launch_decode(const void* q, const void* kc, const void* vc, const int* kv_len, void* o, float* lse,
                                float* ws_o, float* ws_ml, int B, int Hq, int Hkv, int cap, float scale,
                                hipStream_t st) {
  const int NC = (cap + kKC - 1) / kKC;
  const int G = Hq / Hkv;
  hipError_t e;
  // the widest head tile that divides the group: a group of 8 is served from one read of K and V
  if (G % 8 == 0)
    e = launch_chunks<T, D, 8>(q, kc, vc, kv_len, ws_o, ws_ml, B, Hq, Hkv, cap, NC, scale, st);
  else if (G % 4 == 0)
    e = launch_chunks<T, D, 4>(q, kc, vc, kv_len, ws_o, ws_ml, B, Hq, Hkv, cap, NC, scale, st);
  else if (G % 2 == 0)
    e = launch_chunks<T, D, 2>(q, kc, vc, kv_len, ws_o, ws_ml, B, Hq, Hkv, cap, NC, scale, st);
  else
    e = launch_chunks<T, D, 1>(q, kc, vc, kv_len, ws_o, ws_ml, B, Hq, Hkv, cap, NC, scale, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((attn_decode_combine_kernel<T, D>), dim3(Hq, B), dim3(D), 0, st, ws_o, ws_ml, kv_len, (T*)o, lse,
                     Hq, cap, NC);
  return hipGetLastError();
}

}  // namespace pra

extern "C" {

int pra_attn_decode_chunk() { return pra::kKC; }

// fp32 words of workspace: partial outputs [B][Hq][NC][D] followed by (max, sum) [B][Hq][NC][2]
long pra_attn_decode_ws_floats(int B, int Hq, int D, int cap) {
  const long NC = (cap + pra::kKC - 1) / pra::kKC;
  return (long)B * Hq * NC * (D + 2);
}

hipError_t pra_rope_append(int dtype, void* qkv, const void* tab, const int* kv_len, void* k_cache, void* v_cache,
                           int B, int nt, long ld, int Hq, int Hkv, int D, int cap, hipStream_t s) {
  if (B <= 0 || nt <= 0 || cap <= 0 || Hq <= 0 || Hkv <= 0 || D % 8 || ld % 8 || (long)cap + nt > 0x7fffffffL)
    return hipErrorInvalidValue;
  const long items = (long)B * nt * (Hq + 2 * Hkv) * D / 8;
  long grid = (items + 255) / 256;
  if (grid > 2048) grid = 2048;
  PRA_DISPATCH_16BIT(dtype, T,
                     hipLaunchKernelGGL((pra::rope_append_kernel<T>), dim3((unsigned)grid), dim3(256), 0, s, (T*)qkv,
                                        (const float2*)tab, kv_len, (T*)k_cache, (T*)v_cache, B, nt, ld, Hq, Hkv, D,
                                        cap));
  return hipGetLastError();
}

hipError_t pra_attn_decode(int dtype, const void* q, const void* k_cache, const void* v_cache, const int* kv_len,
                           void* o, float* lse, float* ws, int B, int Hq, int Hkv, int D, int cap, float scale,
                           hipStream_t s) {
  if (B <= 0 || cap <= 0 || Hkv <= 0 || Hq % Hkv || B > 65535 || Hq > 65535) return hipErrorInvalidValue;
  const long NC = (cap + pra::kKC - 1) / pra::kKC;
  float* ws_o = ws;
  float* ws_ml = ws + (long)B * Hq * NC * D;
  PRA_DISPATCH_16BIT(dtype, T, {
    if (D == 64) return pra::launch_decode<T, 64>(q, k_cache, v_cache, kv_len, o, lse, ws_o, ws_ml, B, Hq, Hkv, cap, scale, s);
    if (D == 128) return pra::launch_decode<T, 128>(q, k_cache, v_cache, kv_len, o, lse, ws_o, ws_ml, B, Hq, Hkv, cap, scale, s);
    return hipErrorInvalidValue;
  });
  return hipErrorInvalidValue;
}

// The combine kernel alone, over partials that another chunk kernel wrote in this file's workspace layout
// with this file's chunk length (attention_decode_fp8.hip).
hipError_t pra_attn_decode_combine(int dtype, const float* ws_o, const float* ws_ml, const int* kv_len, void* o,
                                   float* lse, int B, int Hq, int D, int cap, int NC, hipStream_t s) {
  if (B <= 0 || Hq <= 0 || B > 65535 || NC != (cap + pra::kKC - 1) / pra::kKC) return hipErrorInvalidValue;
  PRA_DISPATCH_16BIT(dtype, T, {
    if (D == 64)
      hipLaunchKernelGGL((pra::attn_decode_combine_kernel<T, 64>), dim3(Hq, B), dim3(64), 0, s, ws_o, ws_ml, kv_len,
                         (T*)o, lse, Hq, cap, NC);
    else if (D == 128)
      hipLaunchKernelGGL((pra::attn_decode_combine_kernel<T, 128>), dim3(Hq, B), dim3(128), 0, s, ws_o, ws_ml, kv_len,
                         (T*)o, lse, Hq, cap, NC);
    else
      return hipErrorInvalidValue;
  });
  return hipGetLastError();
}
}
