// Multi-token KV-cache append ("extend") attention over an MXFP4 cache for gfx950: bf16 / fp16 queries,
// head_dim 64 / 128, native GQA. attention_extend_fp8.hip with one difference: how K and V reach the LDS image.
//
// The cache (attention_decode_fp4.hip documents the format): k, v uint8 [B][cap][Hkv][D / 2] of e2m1 nibble
// pairs (element 2i in the low nibble of byte i), k_scale, v_scale uint8 [B][cap][Hkv][D / 32], byte = e + 127,
// one per block of 32 columns. The T new tokens' rows are in the cache already (rope_append_fp4 with T tokens
// runs first): query t of sequence b attends to the DEQUANTIZED rows 0 .. min(kv_len[b] + t, cap - 1), its own
// and the other new rows included. The cache is the single source of K and V, as for a decode step.
//
// Staging (Stage4). A 64-key tile is 64 x D / 2 bytes, a quarter of the 16-bit tile: 64 * D / 32 loads of 16 B,
// each exactly one MX block (32 elements) with its one scale byte. At D 128 that is one load per thread for K
// and one for V; at D 64 waves 0 and 1 load and waves 2 and 3 stage nothing (wave-uniform). Between the global
// load and the LDS store the nibbles are converted in registers by v_cvt_scalef32_pk_{bf16,f16}_fp4 with the
// block's 2^e as the scale operand (built as an fp32 bit pattern: byte << 23, and 0x00400000 = 2^-127 for byte
// 0), so what lands in LDS is the dequantized tile in the swizzled 16-bit image of attn_common.h: every nibble
// is converted once per block, never per MFMA operand read, and LaneOff::rowk / the transposed
// ds_read_b64_tr_b16 reads of V work as they are. One word of 8 nibbles becomes one 16-B chunk of the image,
// so a lane produces the four chunks 4 blk .. 4 blk + 3 of its row: one whole 64-B sub-tile row. A stage holds
// 4 + 1 registers per tensor where the 16-bit stage holds 32 at D 128; one tile is staged ahead, like the
// other extend kernels (two ahead is not built and not measured).
//
// Store lanes. The image (lay_byte) puts chunk ch of row r at
//   16 D (r >> 3) + 512 (ch >> 2) + 64 (r & 7) + 16 ((ch & 3) ^ ((r >> 2) & 3)).
// A ds_write_b128 is serviced in phases of 8 lanes over 128 B of banks. Store j of a lane writes chunk
// ch = 4 blk + j, so modulo 128 its address is 64 (r & 1) + 16 (j ^ ((r >> 2) & 3)): the terms 16 D (r >> 3),
// 512 blk and 64 (r & 6) are multiples of 128. The 8 lanes of a phase therefore share blk and row bit 1 and
// take the rows r = base + a + 4 s, a = lane & 1, s = (lane >> 1) & 3 (base has bits 0, 2 and 3 clear): a picks
// the 64-B half and s -> j ^ s is a bijection of the four slots, 128 distinct bytes, conflict-free for every j.
// Row-major (8 lanes = 8 blocks of 2 or 4 rows) would put all 8 lanes on at most two rows' slots. The other
// lane bits: h = lane >> 3 gives blk = h % (D / 32), then row bit 1, then (D 64) row bit 4; a wave covers 64 /
// (D / 32) whole cache rows (64 B or 32 B of contiguous bytes each), the four waves consecutive row groups.
//
// Values. e2m1 x 2^e has two significant bits and is exact in bf16 and in fp16 for every row that
// kv_quantize_fp4 / rope_append_fp4 wrote from that dtype: the block's e is at most 2 below its maximum's
// exponent, and a value of the dtype rounds to a code whose value x 2^e is again a multiple of the dtype's
// smallest subnormal. The convert keeps subnormal results (0.5 x 2^-127 comes out as the bf16 2^-128, 4 x 2^-26
// as the fp16 2^-24; seen on MI355X). So the LDS image is what Stage::store writes for the dequantized 16-bit
// cache, bit for bit, and from there on the kernel has the 16-bit kernel's rounding points and no more: for a
// fixed split its o and lse equal attn_extend's on that cache (tests/test_extend_fp4_gpu.py). One corner is
// outside the op's contract: a block whose maximum rounds up to 4 x 2^e beyond the dtype's range, which is
// 2^128 for bf16 (maximum above 1.75 x 2^127, noted in attention_decode_fp4.hip) and 65536 for fp16
// (|x| > 57344). There the convert does not saturate: it returns the dtype's infinity (seen on MI355X for both),
// where the decode kernel, which scales in fp32, still holds a finite 65536 for fp16.
//
// Load bounds are the 16-bit kernel's: nothing at or beyond min(kv_len[b] + T, cap) is loaded, neither nibbles
// nor scale bytes; nibbles 0 and scale 1 stand in (and are masked). Whatever the tail holds cannot reach an
// output.
//
// One kernel serves both arms. SPLIT = false is the single pass (WS = 1: four 32-row sub-tiles, the block
// walks every key tile of its rows, the row-per-lane epilogue writes o / lse). SPLIT = true is the key
// split: a block belongs to (row tile, kv head, sequence, chunk of kExtendChunk keys), the WS waves (4 / 2
// / 1) that share a 32-row sub-tile divide the chunk's key tiles and fold their states in wave order, and
// the fp32 partial goes to the workspace that attention_extend_split.hip's extend_combine_kernel merges in
// ascending chunk order. The plan is extend_plan (attn_extend_plan.h), unchanged: shapes and CU count only.
// No atomics, one fixed summation order per arm: for a fixed split setting a sequence's o / lse are a pure
// function of its own q, cache rows, kv_len[b] and T, with the same bits from run to run.
// Compiled with attention_extend_fp8.hip's flags (-fno-honor-nans, no SLP): no NaN is formed.
// From the first MFMA on, the kernel body is extend_fp8_kernel's (and so extend_split_kernel's and, with SPLIT =
// false, extend_fwd_kernel's) line for line: a copy, because those kernels' device code must stay as it is. A
// change to the tile loop, the wave fold or the partial store goes into all four files.
#include "attn_common.h"
#include "common.h"
#include "attn_launch.h"

namespace pra {
namespace attn {

constexpr float kFp4NoMax = -1e30f;  // attention_extend.hip's kNoMax

// 2^(byte - 127) as fp32; byte 0 is the subnormal 2^-127 (attention_decode_fp4.hip's fp4_scale_of)
__device__ __forceinline__ float x4_scale_of(uint32_t byte) {
  return __uint_as_float(byte != 0u ? byte << 23 : 0x00400000u);
}

// the 8 nibbles of word w times sc as one 16-B chunk of 16-bit values (exact for the cache's rows)
template <typename T>
__device__ __forceinline__ uint4 cvt8_fp4(uint32_t w, float sc);
template <>
__device__ __forceinline__ uint4 cvt8_fp4<__bf16>(uint32_t w, float sc) {
  return make_uint4(__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, 0)),
                    __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, 1)),
                    __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, 2)),
                    __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, 3)));
}
template <>
__device__ __forceinline__ uint4 cvt8_fp4<_Float16>(uint32_t w, float sc) {
  return make_uint4(__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, sc, 0)),
                    __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, sc, 1)),
                    __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, sc, 2)),
                    __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, sc, 3)));
}

// Stage a 64 x D tile of nibbles and its 64 x D / 32 block scales into registers: one MX block per thread.
// store() converts and writes the dequantized 16-bit tile into attn_common.h's LDS image. 256 threads, of which
// 64 * D / 32 stage (all at D 128, waves 0 and 1 at D 64).
template <typename T, int D>
struct Stage4 {
  static constexpr int NB = D / 32;    // MX blocks (16-B loads) of a row
  static constexpr int RW = 64 / NB;   // rows covered by one wave's loads
  static constexpr int NLD = 64 * NB;  // threads that stage
  static_assert(NLD <= 256 && NLD % 64 == 0, "one block per thread, whole waves");
  uint4 r;
  uint32_t e;
  __device__ __forceinline__ static void rb(int& row, int& blk) {
    const int l = threadIdx.x & 63, h = l >> 3, rest = h / NB;
    blk = h % NB;
    row = RW * (threadIdx.x >> 6) + (l & 1) + 4 * ((l >> 1) & 3) + 2 * (rest & 1) + 16 * (rest >> 1);
  }
  // g: the (sequence, kv head)'s first byte; gs: its first scale byte; ld: bytes between rows; lds: scale bytes
  // between rows
  __device__ __forceinline__ void load(const uint8_t* g, const uint8_t* gs, long ld, long lds, int row0,
                                       int nrows_valid) {
    int row, blk;
    rb(row, blk);
    r = make_uint4(0, 0, 0, 0);
    e = 127u;
    if ((NLD == 256 || threadIdx.x < NLD) && row0 + row < nrows_valid) {
      r = *reinterpret_cast<const uint4*>(g + (long)(row0 + row) * ld + blk * 16);
      e = gs[(long)(row0 + row) * lds + blk];
    }
  }
  __device__ __forceinline__ void store(T* tile) const {
    if (NLD != 256 && threadIdx.x >= NLD) return;  // wave-uniform
    int row, blk;
    rb(row, blk);
    const float s = x4_scale_of(e);
    char* t = reinterpret_cast<char*>(tile);
    *reinterpret_cast<uint4*>(t + lay_byte<D>(row, 4 * blk)) = cvt8_fp4<T>(r.x, s);
    *reinterpret_cast<uint4*>(t + lay_byte<D>(row, 4 * blk + 1)) = cvt8_fp4<T>(r.y, s);
    *reinterpret_cast<uint4*>(t + lay_byte<D>(row, 4 * blk + 2)) = cvt8_fp4<T>(r.z, s);
    *reinterpret_cast<uint4*>(t + lay_byte<D>(row, 4 * blk + 3)) = cvt8_fp4<T>(r.w, s);
  }
};

// SPLIT: grid (row tiles x Hkv x B) x NC, the chunk fastest; else grid row tiles x Hkv x B (NC = 1). The row
// tile is slowest and descending: late row tiles walk the most keys. Q rows are [B * nt][ldq]. SPLIT writes
// WO fp32 [B][nt][Hq][NC][D] and WML fp32 [B][nt][Hq][NC][2] = (max, sum); else O [B][nt][Hq][D] and LSE.
// lds: scale bytes between two cache rows.
template <typename T, int D, int WS, bool SPLIT>
__global__ __launch_bounds__(256, 2) void extend_fp4_kernel(const T* __restrict__ Q, const uint8_t* __restrict__ K,
                                                            const uint8_t* __restrict__ V,
                                                            const uint8_t* __restrict__ KS,
                                                            const uint8_t* __restrict__ VS, T* __restrict__ O,
                                                            float* __restrict__ LSE, float* __restrict__ WO,
                                                            float* __restrict__ WML, const int* __restrict__ KVLEN,
                                                            int nt, int Hq, int Hkv, int cap, int NC, long ldq,
                                                            long lds, float scale_log2) {
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

  const long ldkv = (long)Hkv * (D / 2);  // bytes
  const uint8_t* Kb = K + (long)b * cap * ldkv + hk * (D / 2);
  const uint8_t* Vb = V + (long)b * cap * ldkv + hk * (D / 2);
  const uint8_t* KSb = KS + (long)b * cap * lds + hk * (D / 32);
  const uint8_t* VSb = VS + (long)b * cap * lds + hk * (D / 32);
  const T* Qr = Q + ((long)b * nt + t) * ldq + hq * D + 8 * h2;

  LaneOff<T, D> lo;
  lo.init(lane);
  V8<T> qf[NKS];
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) qf[ks] = *reinterpret_cast<const V8<T>*>(Qr + 16 * ks);

  f32x16 o[NDB];
#pragma unroll
  for (int i = 0; i < NDB; ++i) o[i] = f32x16{};
  float m_i = kFp4NoMax, l_i = 0.f;

  const int nkt = (klast - kc0) / KT + 1;  // tiles of this block: at least one
  const int nvalid = bend + 1;             // rows of the cache the block may load (<= min(len + nt, cap))

  Stage4<T, D> sk, sv;
  sk.load(Kb, KSb, ldkv, lds, kc0, nvalid);
  sv.load(Vb, VSb, ldkv, lds, kc0, nvalid);
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
      sk.load(Kb, KSb, ldkv, lds, k0 + KT, nvalid);
      sv.load(Vb, VSb, ldkv, lds, k0 + KT, nvalid);
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
  // barrier: the tile buffers are free. A wave that took no tile holds (kFp4NoMax, 0, 0) and folds in with
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

using WaveSplit4 = One<1, 2, 4>;

}  // namespace attn
}  // namespace pra

extern "C" hipError_t pra_attn_extend_fp4(int dtype, const void* q, long ldq, const void* k_cache, const void* v_cache,
                                          const uint8_t* k_scale, const uint8_t* v_scale, long ld_scale,
                                          const int* kv_len, void* o, float* lse, float* ws, int B, int T, int Hq,
                                          int Hkv, int D, int cap, float scale, int split, hipStream_t s) {
  using namespace pra::attn;
  if (q == nullptr || k_cache == nullptr || v_cache == nullptr || k_scale == nullptr || v_scale == nullptr ||
      kv_len == nullptr || o == nullptr || lse == nullptr)
    return hipErrorInvalidValue;
  if (B <= 0 || T <= 0 || cap <= 0 || Hq <= 0 || Hkv <= 0 || Hq % Hkv || (D != 64 && D != 128) || ldq % 8 ||
      ldq < (long)Hq * D || (long)T * (Hq / Hkv) > 0x7fffffffL - 128 || (long)cap > 0x7fffffffL / 2 || split < -1 ||
      split > 1 || ld_scale < (long)Hkv * (D / 32))
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
            hipLaunchKernelGGL((extend_fp4_kernel<E, d(), 1, false>), grid, block, 0, s, (const E*)q, kc, vc, k_scale,
                               v_scale, (E*)o, lse, (float*)nullptr, (float*)nullptr, kv_len, T, Hq, Hkv, cap, 1, ldq,
                               ld_scale, sl2);
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
          hipLaunchKernelGGL((extend_fp4_kernel<E, d(), w(), true>), grid, block, 0, s, (const E*)q, kc, vc, k_scale,
                             v_scale, (E*)nullptr, (float*)nullptr, ws_o, ws_ml, kv_len, T, Hq, Hkv, cap, NC, ldq,
                             ld_scale, sl2);
        },
        HeadDim{D}, WaveSplit4{pl.ws_waves});
    return found ? hipGetLastError() : hipErrorInvalidValue;
  });
  if (e != hipSuccess) return e;
  return pra_attn_extend_combine(dtype, ws_o, ws_ml, kv_len, o, lse, B, T, Hq, D, cap, NC, s);
}
