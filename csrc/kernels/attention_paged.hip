// Paged KV cache for gfx950: the append, prompt-store, decode and extend kernels over a pool of fixed-size
// pages and a per-sequence block table (bf16 / fp16, head_dim 64 / 128, native GQA).
//
// Layout, per layer: k_pool, v_pool [n_pages][page][Hkv][D] contiguous, page 64, 128 or 256 keys: the sizes that
// divide the decode chunk (kKC = 256) and the extend chunk (kExtendChunk = 512) and are multiples of the 64-key
// tile. block_table int32 [B][P], P = ceil(cap / page), on the device: logical key j of sequence b is row
// j % page of page block_table[b][j / page]. cap is the logical capacity (no multiple of page needed), one table
// serves every layer, two sequences may name the same page. An entry < 0 or >= n_pages is unmapped: a store to
// it stores nothing, a load from it yields zeros and the key is masked, and no address is ever formed from it
// (the paged form of the kv_len clamps). kv_len stays int32 [B] on the device, clamped as in the dense
// kernels; no launch argument depends on a host copy of it or of the table.
//
// Bit contract. Chunk and tile boundaries stay a function of the key position alone and every sum keeps its
// terms and their order, so each kernel here returns, bit for bit, what its dense counterpart returns on the
// gathered cache k[b][j] = k_pool[block_table[b][j / page]][j % page] (attn_extend: at the same split
// setting). The result does not depend on which physical pages are used, on n_pages or on what the rest of
// the pool holds: pages a sequence does not name, and rows at or beyond its bound, are never loaded.
//
// The page indirection puts a dependent load (table entry, then the k / v address) in front of every cache
// read. How each kernel keeps it off the critical path:
//  * attn_decode_chunk_paged_kernel. A workgroup owns (sequence, kv-head tile, 256-key chunk): at most
//    256 / page <= 4 table entries, workgroup-uniform, read once with scalar loads before anything else. A
//    step of KPB rows (32 at D 128, 64 at D 64) lies inside one page, so its page base is a uniform select
//    among those entries and, as in the dense kernel, all of the chunk's K and V loads are issued before the
//    first use. A chunk at or beyond kv_len[b] leaves before it touches the table or the pool.
//  * extend_fwd_paged_kernel (single pass). A 64-key tile lies inside one page. The entry of tile kt + 2 is
//    fetched (uniform, index clamped into [0, P - 1]) while tile kt + 1 is being register-staged, so the
//    address of a staging load never waits on a table load issued in the same iteration.
//  * extend_split_paged_kernel. A block's chunk spans 512 / page <= 8 entries, read once at block start.
//  * rope_append_paged_kernel, kv_store_paged_kernel: one entry per 16-B item, latency hidden by occupancy.
// The merges are the dense ones: pra_attn_decode_combine and pra_attn_extend_combine over the unchanged
// workspace layouts.
//
// Compiled with the flags of attention_extend_split.hip (-fno-honor-nans: no NaN is formed).
// The tile loop now exists five times and is kept in step by hand: attention_extend.hip,
// attention_extend_split.hip, attention_extend_fp8.hip (both arms) and the two extend kernels here, and a sixth
// time, without masks, in attention_decode_shared.hip; the decode chunk kernel is a second copy of
// attention_decode.hip's, rope_append_paged_kernel of its rope_append_kernel.
// attention_decode_shared.hip (shared-prefix decode) launches the decode chunk kernel's SH = true instantiation
// through decode_chunks as its per-sequence remainder; what the files share is in attn_paged.h.
#include "attn_common.h"
#include "common.h"
#include "attn_launch.h"
#include "attn_paged.h"

#include <math.h>

namespace pra {
namespace paged {

using namespace pra::attn;

constexpr int kDecWaves = 8;
constexpr int kDecThreads = 64 * kDecWaves;

// attention_decode.hip's helpers, same expressions (the bits must match)
__device__ __forceinline__ void rot_pair(float a, float b, float c, float s, float& o0, float& o1) {
  o0 = __builtin_fmaf(a, c, -(b * s));
  o1 = __builtin_fmaf(a, s, b * c);
}
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
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));
template <typename T>
__device__ __forceinline__ float dot8(const uint4& a, const uint4& b);
template <>
__device__ __forceinline__ float dot8<__bf16>(const uint4& a, const uint4& b) {
  float c = 0.f;
  c = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2_t, a.x), __builtin_bit_cast(bf16x2_t, b.x), c, false);
  c = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2_t, a.y), __builtin_bit_cast(bf16x2_t, b.y), c, false);
  c = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2_t, a.z), __builtin_bit_cast(bf16x2_t, b.z), c, false);
  c = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2_t, a.w), __builtin_bit_cast(bf16x2_t, b.w), c, false);
  return c;
}
template <>
__device__ __forceinline__ float dot8<__half>(const uint4& a, const uint4& b) {
  float c = 0.f;
  c = __builtin_amdgcn_fdot2(__builtin_bit_cast(f16x2_t, a.x), __builtin_bit_cast(f16x2_t, b.x), c, false);
  c = __builtin_amdgcn_fdot2(__builtin_bit_cast(f16x2_t, a.y), __builtin_bit_cast(f16x2_t, b.y), c, false);
  c = __builtin_amdgcn_fdot2(__builtin_bit_cast(f16x2_t, a.z), __builtin_bit_cast(f16x2_t, b.z), c, false);
  c = __builtin_amdgcn_fdot2(__builtin_bit_cast(f16x2_t, a.w), __builtin_bit_cast(f16x2_t, b.w), c, false);
  return c;
}

// ---- append -----------------------------------------------------------------------------
// rope_append_kernel with the row address resolved through the table. qkv [B * nt][ld]: q | k | v, one lane
// per 8 columns. ps = log2(page). A token whose page is unmapped stores nothing; its q is still rotated.
template <typename T>
__global__ __launch_bounds__(256) void rope_append_paged_kernel(T* __restrict__ qkv, const float2* __restrict__ tab,
                                                                const int* __restrict__ kv_len, T* __restrict__ kp,
                                                                T* __restrict__ vp, const int* __restrict__ bt, int B,
                                                                int nt, long ld, int Hq, int Hkv, int D, int cap, int ps,
                                                                int P, int n_pages) {
  const int nq = Hq * D, nk = Hkv * D;
  const int vpr = (nq + 2 * nk) / 8;
  const long total = (long)B * nt * vpr;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const long r = idx / vpr;  // row b * nt + t
    const int b = (int)(r / nt);
    const int col = (int)(idx - r * vpr) * 8;
    const int at = min(max(kv_len[b], 0), cap) + (int)(r - (long)b * nt);  // <= cap + nt - 1
    const int pos = min(at, cap - 1);
    T* p = qkv + r * ld + col;
    float v[8];
    load8<T>(p, v);
    bool keep = false;
    long row = 0;  // pool row of this token, in elements
    if (col >= nq && (at < cap || nt == 1)) {  // one token: the clamped row is overwritten
      const int e = bt[(long)b * P + (pos >> ps)];  // pos <= cap - 1: inside the table row
      keep = mapped(e, n_pages);
      if (keep) row = (((long)e << ps) + (pos & ((1 << ps) - 1))) * nk;
    }
    if (col >= nq + nk) {
      if (keep) store8<T>(vp + row + (col - nq - nk), v);  // exact copy
      continue;
    }
    const int pi = (col % D) / 2;
    const float4* tp = reinterpret_cast<const float4*>(tab + (size_t)pos * (D / 2) + pi);
    const float4 cs01 = tp[0], cs23 = tp[1];
    const float c[4] = {cs01.x, cs01.z, cs23.x, cs23.z};
    const float s[4] = {cs01.y, cs01.w, cs23.y, cs23.w};
    float o[8];
#pragma unroll
    for (int k = 0; k < 4; ++k) rot_pair(v[2 * k], v[2 * k + 1], c[k], s[k], o[2 * k], o[2 * k + 1]);
    if (col < nq)
      store8<T>(p, o);
    else if (keep)
      store8<T>(kp + row + (col - nq), o);
  }
}

// The prompt's k / v rows [B * S][ld] (views of the fused QKV activation, nk = Hkv * D columns each) into
// logical rows 0 .. S - 1: one lane per 16 B of a k row and the same 16 B of the v row. Rows on an
// unmapped page (prompt padding beyond a sequence's allocation) go nowhere.
__global__ __launch_bounds__(256) void kv_store_paged_kernel(const uint4* __restrict__ k, const uint4* __restrict__ v,
                                                             uint4* __restrict__ kp, uint4* __restrict__ vp,
                                                             const int* __restrict__ bt, int S, long ld8, int nk8,
                                                             long total, int ps, int P, int n_pages) {
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const long r = idx / nk8;  // row b * S + s
    const int c = (int)(idx - r * nk8);
    const int b = (int)(r / S), s = (int)(r - (long)b * S);
    const int e = bt[(long)b * P + (s >> ps)];  // s < S <= cap
    if (!mapped(e, n_pages)) continue;
    const long row = (((long)e << ps) + (s & ((1 << ps) - 1))) * nk8 + c;
    kp[row] = k[r * ld8 + c];
    vp[row] = v[r * ld8 + c];
  }
}

// ---- decode -----------------------------------------------------------------------------
// attn_decode_chunk_kernel over the pool. grid (NC, Hkv * (G / GT), B); partials as there: ws_o
// [B][Hq][NC][D] fp32 (unnormalised), ws_ml [B][Hq][NC][2] = (max in log2 units, sum).
// SH: the per-sequence remainder of the shared-prefix decode (attention_decode_shared.hip). A chunk below the
// effective shared length of b's group belongs to decode_shared_chunk_kernel: the workgroup leaves at once and
// writes nothing. Nothing else differs, and without SH the two extra arguments are not read.
template <typename T, int D, int GT, bool SH>
__global__ __launch_bounds__(kDecThreads) void attn_decode_chunk_paged_kernel(
    const T* __restrict__ q, const T* __restrict__ kp, const T* __restrict__ vp, const int* __restrict__ bt,
    const int* __restrict__ kv_len, float* __restrict__ ws_o, float* __restrict__ ws_ml, int Hq, int Hkv, int cap,
    int NC, int ps, int P, int n_pages, float scale_log2, const int* __restrict__ shared_len, int gsz) {
  constexpr int LPK = D / 8;
  constexpr int KPW = 64 / LPK;
  constexpr int KPB = kDecWaves * KPW;
  constexpr int STEPS = kKC / KPB;  // rows of K (and of V) per lane
  static_assert(kKC % KPB == 0 && STEPS >= 1 && 64 % KPB == 0, "a step must lie inside a 64-key page");
  __shared__ float s_p[kKC * GT];              // [key][g]: scores, then probabilities
  __shared__ float s_red[kDecWaves * GT * D];  // [wave][g][d]: per-wave P.V

  const int b = blockIdx.z;
  const int G = Hq / Hkv;
  const int tiles = G / GT;
  const int hkv = blockIdx.y / tiles;
  const int h0 = hkv * G + (blockIdx.y - hkv * tiles) * GT;  // first query head served here
  const int chunk = blockIdx.x;
  const int c0 = chunk * kKC;
  if constexpr (SH) {  // workgroup-uniform; its loads need no kv_len[b], so the exit costs no further latency
    if (shared_prefix_covers(shared_len, kv_len, b / gsz, gsz, cap, c0)) return;
  }
  const int len = min(max(kv_len[b], 0), cap);
  if (c0 >= len) return;  // wave-uniform: no table entry, nothing of the pool read, nothing written

  // the chunk's table entries (c0 is a multiple of the page): uniform addresses, scalar loads
  // (indices clamped into the row, so the four loads issue back to back; entries past the chunk or the row
  // become -1). Named scalars, not an array: the selects below must fold, not index memory.
  const int* btb = bt + (long)b * P;
  const int p0 = c0 >> ps, npc = kKC >> ps;
  const int l0 = btb[p0], l1 = btb[min(p0 + 1, P - 1)], l2 = btb[min(p0 + 2, P - 1)], l3 = btb[min(p0 + 3, P - 1)];
  const int e0 = l0;  // c0 < len <= cap: page p0 is inside the row
  const int e1 = (1 < npc && p0 + 1 < P) ? l1 : -1;
  const int e2 = (2 < npc && p0 + 2 < P) ? l2 : -1;
  const int e3 = (3 < npc && p0 + 3 < P) ? l3 : -1;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int part = lane % LPK;  // which 8 columns of the row
  const int ks = lane / LPK;    // which row of the wave-load
  const int pm = (1 << ps) - 1;
  const long tok_stride = (long)Hkv * D;
  const T* kbase = kp + (long)hkv * D + part * 8;
  const T* vbase = vp + (long)hkv * D + part * 8;

  // every load of the chunk, K first; a key at or beyond len, or on an unmapped page, is never loaded
  // the step's page is uniform (scalar registers); the lane adds its row inside the step
  uint4 kraw[STEPS], vraw[STEPS];
  const int lrow = wave * KPW + ks;
  auto step_row = [&](int st, bool& ok) -> long {
    const int i6 = (st * KPB) >> 6, i7 = (st * KPB) >> 7;  // constants once the step loops are unrolled
    const int a = sel(i6 == 0, e0, sel(i6 == 1, e1, sel(i6 == 2, e2, e3)));
    const int e = sel(ps == 6, a, sel(ps == 7, sel(i7 == 0, e0, e1), e0));
    ok =c0 + st * KPB + lrow < len && mapped(e, n_pages);
    return ok ? (long)((e << ps) + ((st * KPB) & pm)) + lrow : 0;  // e < n_pages: n_pages * page fits an int
  };
#pragma unroll
  for (int st = 0; st < STEPS; ++st) {
    bool ok;
    const long r = step_row(st, ok);
    kraw[st] = make_uint4(0u, 0u, 0u, 0u);
    if (ok) kraw[st] = *reinterpret_cast<const uint4*>(kbase + r * tok_stride);
  }
#pragma unroll
  for (int st = 0; st < STEPS; ++st) {
    bool ok;
    const long r = step_row(st, ok);
    vraw[st] = make_uint4(0u, 0u, 0u, 0u);
    if (ok) vraw[st] = *reinterpret_cast<const uint4*>(vbase + r * tok_stride);
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
          bool valid;
          step_row(st, valid);
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
    float m = kNoMax;
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

// ---- extend -----------------------------------------------------------------------------
// The tile loop body shared by the two extend kernels below is written out in each, as in the dense files.

// extend_fwd_kernel over the pool. grid row tiles x Hkv x B, the row tile slowest and descending.
template <typename T, int D>
__global__ __launch_bounds__(256, 2) void extend_fwd_paged_kernel(const T* __restrict__ Q, const T* __restrict__ K,
                                                                  const T* __restrict__ V, const int* __restrict__ BT,
                                                                  T* __restrict__ O, float* __restrict__ LSE,
                                                                  const int* __restrict__ KVLEN, int nt, int Hq, int Hkv,
                                                                  int cap, int ps, int P, int n_pages, long ldq,
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

  const int* BTb = BT + (long)b * P;
  const int pm = (1 << ps) - 1;
  int e_cur = BTb[0];                      // tile 0's page
  int e_nxt = BTb[min(KT >> ps, P - 1)];   // tile 1's

  const int len = min(max(KVLEN[b], 0), cap);
  const int kend = min(len + t, cap - 1);                              // this row's last visible key
  const int bend = min(len + min(r0 + QT - 1, R - 1) / G, cap - 1);    // the block's
  const bool active = rw < R;                                          // wave-uniform: the wave has a real row
  const int wlo = min(len + min(rw, R - 1) / G, cap - 1);              // the wave's smallest bound
  const int whi = active ? min(len + min(rw + 31, R - 1) / G, cap - 1) : -1;  // and its largest

  const long ldkv = (long)Hkv * D;
  const T* Kh = K + hk * D;
  const T* Vh = V + hk * D;
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
  const int nvalid = bend + 1;    // logical rows the block may load (<= min(len + nt, cap))

  // a tile at logical key k0 on page entry e: rows [0, nvalid - k0) of the page rows from k0 % page on; an
  // unmapped page stages zeros from no address at all
  Stage<T, D, KT, NW * 64> sk, sv;
  auto stage = [&](int e, int k0) {
    const bool ok = mapped(e, n_pages);
    const long prow = ok ? ((long)e << ps) + (k0 & pm) : 0;
    const int nv = ok ? nvalid - k0 : 0;
    sk.load(Kh + prow * ldkv, ldkv, 0, nv);
    sv.load(Vh + prow * ldkv, ldkv, 0, nv);
  };
  stage(e_cur, 0);
  sk.store(smem);
  sv.store(smem + TILE);
  __syncthreads();

  auto body = [&](auto cc, int kt) {
    constexpr int CUR = decltype(cc)::value;
    const T* Kt = smem + 2 * CUR * TILE;
    const T* Vt = Kt + TILE;
    const int k0 = kt * KT;
    const bool more = kt + 1 < nkt;
    const int e1 = e_nxt;  // tile kt + 1's entry, fetched an iteration ago
    if (more) stage(e1, k0 + KT);
    e_nxt = BTb[min((k0 + 2 * KT) >> ps, P - 1)];  // tile kt + 2's: in flight under this tile's MFMAs
    if (k0 <= whi && mapped(e_cur, n_pages)) {  // wave-uniform: else wholly after the wave's bounds, or masked
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
    e_cur = e1;
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

// extend_split_kernel over the pool. grid (row tiles x Hkv x B) x NC, the chunk fastest. WO fp32
// [B][nt][Hq][NC][D], WML fp32 [B][nt][Hq][NC][2] = (max, sum): extend_combine_kernel's input.
template <typename T, int D, int WS>
__global__ __launch_bounds__(256, 2) void extend_split_paged_kernel(const T* __restrict__ Q, const T* __restrict__ K,
                                                                    const T* __restrict__ V,
                                                                    const int* __restrict__ BT, float* __restrict__ WO,
                                                                    float* __restrict__ WML,
                                                                    const int* __restrict__ KVLEN, int nt, int Hq,
                                                                    int Hkv, int cap, int NC, int ps, int P, int n_pages,
                                                                    long ldq, float scale_log2) {
  constexpr int NW = 4, KT = 64, NSUB = NW / WS, QT = 32 * NSUB, XC = kExtendChunk;
  constexpr int NKS = D / 16, NDB = D / 32, TILE = KT * D;
  constexpr int NV = 4 * NDB + 1;  // float4 words of one lane's (o, m, l)
  constexpr int NE = XC / 64;      // table entries of a chunk at the smallest page
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
  if (kc0 > bend) return;  // block-uniform: no table entry, nothing read, nothing written
  const int klast = min(kc0 + XC - 1, bend);

  // the chunk's table entries (kc0 is a multiple of the page), read once: uniform addresses
  int ent[NE];
#pragma unroll
  for (int i = 0; i < NE; ++i) {
    const int pi = (kc0 >> ps) + i;  // index clamped into the row: the loads issue back to back
    const int l = BT[(long)b * P + min(pi, P - 1)];
    ent[i] = (i < (XC >> ps) && pi < P) ? l : -1;
  }
  const int pm = (1 << ps) - 1;

  const bool active = rw < R;                                                 // wave-uniform
  const int wlo = min(len + min(rw, R - 1) / G, cap - 1);                     // the wave's smallest bound
  const int whi = active ? min(len + min(rw + 31, R - 1) / G, cap - 1) : -1;  // and its largest

  const long ldkv = (long)Hkv * D;
  const T* Kh = K + hk * D;
  const T* Vh = V + hk * D;
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

  const int nkt = (klast - kc0) / KT + 1;  // tiles of this chunk: 1 .. XC / 64
  const int nvalid = bend + 1;             // logical rows the block may load (<= min(len + nt, cap))

  Stage<T, D, KT, NW * 64> sk, sv;
  auto stage = [&](int e, int k0) {  // as in extend_fwd_paged_kernel
    const bool ok = mapped(e, n_pages);
    const long prow = ok ? ((long)e << ps) + (k0 & pm) : 0;
    const int nv = ok ? nvalid - k0 : 0;
    sk.load(Kh + prow * ldkv, ldkv, 0, nv);
    sv.load(Vh + prow * ldkv, ldkv, 0, nv);
  };
  stage(ent[0], kc0);
  sk.store(smem);
  sv.store(smem + TILE);
  __syncthreads();

  auto body = [&](auto cc, int j) {
    constexpr int CUR = decltype(cc)::value;
    const T* Kt = smem + 2 * CUR * TILE;
    const T* Vt = Kt + TILE;
    const int k0 = kc0 + j * KT;
    const bool more = j + 1 < nkt;
    if (more) stage(pick(ent, ((j + 1) * KT) >> ps), k0 + KT);
    // wave-uniform: the wave's tile, not wholly after its rows' bounds, and on a mapped page
    if (j % WS == kw && k0 <= whi && mapped(pick(ent, (j * KT) >> ps), n_pages)) {
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

  // The waves of a sub-tile, in wave order, through the tile buffers (free after the last barrier): the fold
  // of extend_split_kernel.
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

// ---- host side ----------------------------------------------------------------------------
using WaveSplit = One<1, 2, 4>;
using GroupTile = One<1, 2, 4, 8>;

// Declared in attn_paged.h and also called from attention_decode_shared.hip (its remainder launch): the one
// function of this file that another translation unit links against besides the extern "C" launchers.
hipError_t decode_chunks(int dtype, const void* q, const void* k_pool, const void* v_pool, const int* block_table,
                         const int* kv_len, const int* shared_len, int group_size, float* ws_o, float* ws_ml, int B,
                         int Hq, int Hkv, int D, int cap, int page, int n_pages, float scale, hipStream_t s) {
  const int ps = page_shift(page), P = (cap + page - 1) / page;
  const int NC = (cap + kKC - 1) / kKC;
  const int G = Hq / Hkv;
  // the widest head tile that divides the group, as the dense launcher picks it
  const int GT = G % 8 == 0 ? 8 : G % 4 == 0 ? 4 : G % 2 == 0 ? 2 : 1;
  const dim3 grid(NC, Hkv * (G / GT), B);
  const float sl2 = scale * 1.4426950408889634f;
  PRA_DISPATCH_16BIT(dtype, T, {
    const bool found = pra::dispatch(
        [&](auto d, auto g) {
          auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, dim3(kDecThreads), 0, s, (const T*)q, (const T*)k_pool, (const T*)v_pool,
                               block_table, kv_len, ws_o, ws_ml, Hq, Hkv, cap, NC, ps, P, n_pages, sl2, shared_len,
                               group_size);
          };
          if (shared_len == nullptr)
            launch(attn_decode_chunk_paged_kernel<T, d(), g(), false>);
          else
            launch(attn_decode_chunk_paged_kernel<T, d(), g(), true>);
        },
        HeadDim{D}, GroupTile{GT});
    if (!found) return hipErrorInvalidValue;
  });
  return hipGetLastError();
}

}  // namespace paged
}  // namespace pra

extern "C" {

hipError_t pra_rope_append_paged(int dtype, void* qkv, const void* tab, const int* kv_len, void* k_pool, void* v_pool,
                                 const int* block_table, int B, int nt, long ld, int Hq, int Hkv, int D, int cap,
                                 int page, int n_pages, hipStream_t s) {
  using namespace pra::paged;
  if (qkv == nullptr || tab == nullptr || kv_len == nullptr || !pool_ok(k_pool, v_pool, block_table, cap, page, n_pages))
    return hipErrorInvalidValue;
  if (B <= 0 || nt <= 0 || Hq <= 0 || Hkv <= 0 || (D != 64 && D != 128) || ld % 8 || (long)cap + nt > 0x7fffffffL)
    return hipErrorInvalidValue;
  const int ps = page_shift(page), P = (cap + page - 1) / page;
  const long items = (long)B * nt * (Hq + 2 * Hkv) * D / 8;
  long grid = (items + 255) / 256;
  if (grid > 2048) grid = 2048;
  PRA_DISPATCH_16BIT(dtype, T,
                     hipLaunchKernelGGL((rope_append_paged_kernel<T>), dim3((unsigned)grid), dim3(256), 0, s, (T*)qkv,
                                        (const float2*)tab, kv_len, (T*)k_pool, (T*)v_pool, block_table, B, nt, ld, Hq,
                                        Hkv, D, cap, ps, P, n_pages));
  return hipGetLastError();
}

hipError_t pra_kv_store_paged(int dtype, const void* k, const void* v, long ld, void* k_pool, void* v_pool,
                              const int* block_table, int B, int S, int Hkv, int D, int cap, int page, int n_pages,
                              hipStream_t s) {
  using namespace pra::paged;
  if (k == nullptr || v == nullptr || !pool_ok(k_pool, v_pool, block_table, cap, page, n_pages))
    return hipErrorInvalidValue;
  if ((dtype != pra::kBF16 && dtype != pra::kF16) || B <= 0 || S <= 0 || S > cap || Hkv <= 0 || (D != 64 && D != 128) ||
      ld % 8 || ld < (long)Hkv * D || (long)B * S > 0x7fffffffL / 2)
    return hipErrorInvalidValue;
  const int ps = page_shift(page), P = (cap + page - 1) / page;
  const int nk8 = Hkv * D / 8;
  const long total = (long)B * S * nk8;
  long grid = (total + 255) / 256;
  if (grid > 4096) grid = 4096;
  hipLaunchKernelGGL(kv_store_paged_kernel, dim3((unsigned)grid), dim3(256), 0, s, (const uint4*)k, (const uint4*)v,
                     (uint4*)k_pool, (uint4*)v_pool, block_table, S, ld / 8, nk8, total, ps, P, n_pages);
  return hipGetLastError();
}

hipError_t pra_attn_decode_paged(int dtype, const void* q, const void* k_pool, const void* v_pool,
                                 const int* block_table, const int* kv_len, void* o, float* lse, float* ws, int B,
                                 int Hq, int Hkv, int D, int cap, int page, int n_pages, float scale, hipStream_t s) {
  using namespace pra::paged;
  if (q == nullptr || kv_len == nullptr || o == nullptr || lse == nullptr || ws == nullptr ||
      !pool_ok(k_pool, v_pool, block_table, cap, page, n_pages))
    return hipErrorInvalidValue;
  if (B <= 0 || Hkv <= 0 || Hq <= 0 || Hq % Hkv || B > 65535 || Hq > 65535 || (D != 64 && D != 128) ||
      pra_attn_decode_chunk() != kKC)
    return hipErrorInvalidValue;
  const int NC = (cap + kKC - 1) / kKC;
  float* ws_o = ws;
  float* ws_ml = ws + (long)B * Hq * NC * D;
  const hipError_t e = decode_chunks(dtype, q, k_pool, v_pool, block_table, kv_len, nullptr, 1, ws_o, ws_ml, B, Hq, Hkv,
                                     D, cap, page, n_pages, scale, s);
  if (e != hipSuccess) return e;
  return pra_attn_decode_combine(dtype, ws_o, ws_ml, kv_len, o, lse, B, Hq, D, cap, NC, s);
}

hipError_t pra_attn_extend_paged(int dtype, const void* q, long ldq, const void* k_pool, const void* v_pool,
                                 const int* block_table, const int* kv_len, void* o, float* lse, float* ws, int B, int T,
                                 int Hq, int Hkv, int D, int cap, int page, int n_pages, float scale, int split,
                                 hipStream_t s) {
  using namespace pra::paged;
  if (q == nullptr || kv_len == nullptr || o == nullptr || lse == nullptr ||
      !pool_ok(k_pool, v_pool, block_table, cap, page, n_pages))
    return hipErrorInvalidValue;
  if (B <= 0 || T <= 0 || Hq <= 0 || Hkv <= 0 || Hq % Hkv || (D != 64 && D != 128) || ldq % 8 ||
      ldq < (long)Hq * D || (long)T * (Hq / Hkv) > 0x7fffffffL - 128 || (long)cap > 0x7fffffffL / 2 || split < -1 ||
      split > 1)
    return hipErrorInvalidValue;
  const int ps = page_shift(page), P = (cap + page - 1) / page;
  const float sl2 = scale * kLog2e;
  const pra_attn_extend_plan_t pl = extend_plan(B, T, Hq, Hkv, D, cap, device_cus(), split);
  if (pl.blocks > 0x7fffffffL) return hipErrorInvalidValue;
  const dim3 grid((unsigned)pl.blocks), block(256);
  if (!pl.split)
    return dispatch_16bit(dtype, [&](auto t) {
      using E = decltype(t);
      pra::dispatch(
          [&](auto d) {
            hipLaunchKernelGGL((extend_fwd_paged_kernel<E, d()>), grid, block, 0, s, (const E*)q, (const E*)k_pool,
                               (const E*)v_pool, block_table, (E*)o, lse, kv_len, T, Hq, Hkv, cap, ps, P, n_pages, ldq,
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
          hipLaunchKernelGGL((extend_split_paged_kernel<E, d(), w()>), grid, block, 0, s, (const E*)q, (const E*)k_pool,
                             (const E*)v_pool, block_table, ws_o, ws_ml, kv_len, T, Hq, Hkv, cap, NC, ps, P, n_pages, ldq,
                             sl2);
        },
        HeadDim{D}, WaveSplit{pl.ws_waves});
    return found ? hipGetLastError() : hipErrorInvalidValue;
  });
  if (e != hipSuccess) return e;
  return pra_attn_extend_combine(dtype, ws_o, ws_ml, kv_len, o, lse, B, T, Hq, D, cap, NC, s);
}
}
