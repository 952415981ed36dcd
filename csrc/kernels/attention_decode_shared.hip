// Shared-prefix decode attention over the paged KV cache for gfx950 (bf16 / fp16, head_dim 64 / 128, page 64 /
// 128 / 256, native GQA): one read of the pages that a group of sequences has in common.
//
// The batch is B / n groups of n consecutive sequences (n samples of one prompt, n requests behind one system
// prompt). shared_len[g], int32 on the device, counts the leading tokens whose block-table entries are the same
// for every member of group g. attn_decode_paged streams such a page from HBM once per member; decode attention
// is bound by those bytes. Here the keys below
//   s_eff(g) = floor(min(shared_len[g], cap, min_i clamp(kv_len[g n + i], 0, cap)) / 256) * 256
// (attn_paged.h: shared_prefix_covers; 256 = pra_attn_decode_chunk) are read once per (group, kv head) and serve the
// query heads of all members. Chunk boundaries stay a function of the key position alone; because of the min
// over the members every member attends to every key below s_eff, so the shared kernel masks nothing. Three
// launches, nothing in them depends on a host copy of shared_len, kv_len or the table:
//  * decode_shared_chunk_kernel. A workgroup owns (row tile, kv head, group g, 256-key chunk c) and leaves at
//    once if 256 c >= s_eff(g), before it touches the table or the pool. Its rows are r = i G + h (member i, head
//    h of the kv head's GQA group, G = Hq / Hkv), R = n G in all: with n members the VALU dot products of the
//    per-sequence kernel (G rows) become MFMA work, and the row shape is extend_split_kernel's (token, head)
//    with members in place of tokens: q row r is q[g n + i][hk G + h], a constant stride between members. The
//    design is that kernel's: 4 waves; the chunk's four 64-key tiles are register-staged into attn_common.h's
//    swizzled LDS image, double-buffered; S^T = K Q^T on MFMA 32x32x16 with one query row per lane; the exact
//    running max with the deferred rescale from the finite sentinel; P V with V read through ds_read_b64_tr_b16;
//    the WS = extend_ws_waves(R) waves that share a 32-row sub-tile divide the four tiles and fold their states
//    in wave order through the tile buffers; rows past R repeat the last row and are not stored. K / V
//    addresses come from the table row of member 0 alone: the chunk's 256 / page <= 4 entries, read once at
//    block start with uniform loads and picked with attention_paged.hip's select chain. An unmapped entry
//    stages zeros from no address at all and its tile is skipped.
//    Each row's fp32 partial (unnormalised o[D], max in log2 units with the scale folded in, sum) goes to
//    pra_attn_decode_combine's workspace at (sequence g n + i, head, chunk c), in the units that
//    attn_decode_chunk_kernel writes there.
//  * The per-sequence remainder is attn_decode_chunk_paged_kernel itself (attention_paged.hip), instantiated
//    with SH = true: the one addition is that a workgroup whose chunk lies below s_eff of its sequence's group
//    leaves at once. Not a copy: pra_attn_decode_paged keeps the SH = false instantiation, whose arithmetic is
//    untouched. With s_eff = 0 this kernel does everything, and the result is attn_decode_paged's, bit for bit.
//  * pra_attn_decode_combine, unchanged: every chunk 0 .. ceil(len / 256) - 1 of a (sequence, head) has been
//    written by exactly one of the two kernels.
// No atomics, no workgroup waits on another, one fixed summation order: the same bits from run to run, and a
// group's result does not depend on the rest of the batch or on which physical pages it names.
// Compiled with the flags of attention_extend_split.hip (-fno-honor-nans: no NaN is formed). The tile loop and
// the wave fold are one more hand-synchronised copy of attention_extend_split.hip's (the list is in
// attention_paged.hip's header), here without the masks and the bounds that an append needs.
#include "attn_common.h"
#include "common.h"
#include "attn_launch.h"
#include "attn_paged.h"

namespace pra {
namespace paged {

using namespace pra::attn;

// grid (row tiles x Hkv x groups) x NC, the chunk fastest. Q [B][Hq][D], WO fp32 [B][Hq][NC][D], WML fp32
// [B][Hq][NC][2] = (max, sum), n members per group.
template <typename T, int D, int WS>
__global__ __launch_bounds__(256, 2) void decode_shared_chunk_kernel(
    const T* __restrict__ Q, const T* __restrict__ K, const T* __restrict__ V, const int* __restrict__ BT,
    const int* __restrict__ KVLEN, const int* __restrict__ SHLEN, float* __restrict__ WO, float* __restrict__ WML,
    int n, int Hq, int Hkv, int cap, int NC, int ps, int P, int n_pages, float scale_log2) {
  constexpr int NW = 4, KT = 64, NSUB = NW / WS, QT = 32 * NSUB, NKT = kKC / KT;
  constexpr int NKS = D / 16, NDB = D / 32, TILE = KT * D;
  constexpr int NV = 4 * NDB + 1;  // float4 words of one lane's (o, m, l)
  static_assert((NW - NSUB) * NV * 64 * 16 <= 4 * TILE * (int)sizeof(T), "the merged states must fit the tile buffer");
  static_assert(NKT == 4 && NKT % WS == 0, "a chunk is four tiles, divided evenly among the waves of a sub-tile");
  __shared__ __attribute__((aligned(16))) T smem[4 * TILE];  // K0 V0 K1 V1

  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, h2 = lane >> 5, l32 = lane & 31;
  const int sub = wid / WS, kw = wid % WS;  // the wave's 32-row sub-tile, and its share of the key tiles
  const int G = Hq / Hkv, R = n * G;
  const int nrt = (R + QT - 1) / QT;
  const int c = blockIdx.x % NC;
  const int rest = blockIdx.x / NC;
  const int rt = rest % nrt;
  const int gh = rest / nrt;
  const int hk = gh % Hkv, g = gh / Hkv;
  const int kc0 = c * kKC;
  // block-uniform: no table entry, nothing of the pool read, nothing written. Below s_eff the whole chunk lies
  // under cap and under every member's kv_len.
  if (!shared_prefix_covers(SHLEN, KVLEN, g, n, cap, kc0)) return;

  const int rw = rt * QT + sub * 32;
  const int row = rw + l32;
  const int rc = min(row, R - 1);  // rows past the end repeat the last one and are not stored
  const int mi = rc / G, hq = hk * G + rc % G;
  const long b = (long)g * n + mi;  // the row's sequence
  const bool active = rw < R;       // wave-uniform: the wave has a real row

  // the chunk's table entries from member 0's row (kc0 is a multiple of the page), read once: uniform addresses
  int ent[NKT];
#pragma unroll
  for (int i = 0; i < NKT; ++i) {
    const int pi = (kc0 >> ps) + i;  // index clamped into the row: the loads issue back to back
    const int l = BT[(long)g * n * P + min(pi, P - 1)];
    ent[i] = (i < (kKC >> ps) && pi < P) ? l : -1;
  }
  const int pm = (1 << ps) - 1;

  const long ldkv = (long)Hkv * D;
  const T* Kh = K + hk * D;
  const T* Vh = V + hk * D;
  const T* Qr = Q + (b * Hq + hq) * D + 8 * h2;

  LaneOff<T, D> lo;
  lo.init(lane);
  V8<T> qf[NKS];
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) qf[ks] = *reinterpret_cast<const V8<T>*>(Qr + 16 * ks);

  f32x16 o[NDB];
#pragma unroll
  for (int i = 0; i < NDB; ++i) o[i] = f32x16{};
  float m_i = kNoMax, l_i = 0.f;

  // tile j of the chunk on page entry e: 64 whole rows of the page from (j * 64) % page on (a tile lies inside
  // one page); an unmapped page stages zeros from no address at all
  Stage<T, D, KT, NW * 64> sk, sv;
  auto stage = [&](int j) {
    const int e = pick(ent, (j * KT) >> ps);
    const bool ok = mapped(e, n_pages);
    const long prow = ok ? ((long)e << ps) + ((j * KT) & pm) : 0;
    sk.load(Kh + prow * ldkv, ldkv, 0, ok ? KT : 0);
    sv.load(Vh + prow * ldkv, ldkv, 0, ok ? KT : 0);
  };
  stage(0);
  sk.store(smem);
  sv.store(smem + TILE);
  __syncthreads();

  auto body = [&](auto cc, int j) {
    constexpr int CUR = decltype(cc)::value;
    const T* Kt = smem + 2 * CUR * TILE;
    const T* Vt = Kt + TILE;
    const bool more = j + 1 < NKT;
    if (more) stage(j + 1);
    // wave-uniform: the wave's tile, a real row, a mapped page
    if (j % WS == kw && active && mapped(pick(ent, (j * KT) >> ps), n_pages)) {
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
      float mx = -INFINITY;
#pragma unroll
      for (int r = 0; r < 16; ++r) mx = fmaxf(mx, fmaxf(s0[r], s1[r]));
      mx = half_max(mx) * scale_log2;
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
        s0[r] = fexp2(fmaf(s0[r], scale_log2, -m_i));
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
  body(IC<0>{}, 0);
  body(IC<1>{}, 1);
  body(IC<0>{}, 2);
  body(IC<1>{}, 3);

  // The waves of a sub-tile, in wave order, through the tile buffers (free after the last barrier): the fold of
  // extend_split_kernel. A wave that took no mapped tile holds (kNoMax, 0, 0) and folds in with weight
  // exp2(-1e30 - m) = 0, or 1 onto zeros.
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

  if (kw == 0 && row < R) {
    const long prow = (b * Hq + hq) * NC + c;
    store_rows16_f32<NDB>(o, 1.f, WO + prow * D, h2);
    if (h2 == 0) *reinterpret_cast<float2*>(WML + prow * 2) = make_float2(m_i, l_i);
  }
}

using WaveSplit = One<1, 2, 4>;

}  // namespace paged
}  // namespace pra

extern "C" hipError_t pra_attn_decode_shared_paged(int dtype, const void* q, const void* k_pool, const void* v_pool,
                                                   const int* block_table, const int* kv_len, const int* shared_len,
                                                   void* o, float* lse, float* ws, int B, int group_size, int Hq,
                                                   int Hkv, int D, int cap, int page, int n_pages, float scale,
                                                   hipStream_t s) {
  using namespace pra::paged;
  if (q == nullptr || kv_len == nullptr || shared_len == nullptr || o == nullptr || lse == nullptr || ws == nullptr ||
      (reinterpret_cast<uintptr_t>(ws) & 15) || !pool_ok(k_pool, v_pool, block_table, cap, page, n_pages))
    return hipErrorInvalidValue;
  if (B <= 0 || Hkv <= 0 || Hq <= 0 || Hq % Hkv || B > 65535 || Hq > 65535 || (D != 64 && D != 128) ||
      group_size < 1 || B % group_size || pra_attn_decode_chunk() != kKC)
    return hipErrorInvalidValue;
  const int ps = page_shift(page), P = (cap + page - 1) / page;
  const int NC = (cap + kKC - 1) / kKC;
  float* ws_o = ws;
  float* ws_ml = ws + (long)B * Hq * NC * D;
  const long R = (long)group_size * (Hq / Hkv);  // rows of a (group, kv head)
  if (R > 0x7fffffffL - 128) return hipErrorInvalidValue;
  const int ws_waves = extend_ws_waves(R);
  const long rows = 128 / ws_waves;  // rows of a block
  const long blocks = (R + rows - 1) / rows * Hkv * (B / group_size) * NC;
  if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
  const float sl2 = scale * kLog2e;
  hipError_t e = dispatch_16bit(dtype, [&](auto t) {
    using E = decltype(t);
    const bool found = pra::dispatch(
        [&](auto d, auto w) {
          hipLaunchKernelGGL((decode_shared_chunk_kernel<E, d(), w()>), dim3((unsigned)blocks), dim3(256), 0, s,
                             (const E*)q, (const E*)k_pool, (const E*)v_pool, block_table, kv_len, shared_len, ws_o,
                             ws_ml, group_size, Hq, Hkv, cap, NC, ps, P, n_pages, sl2);
        },
        HeadDim{D}, WaveSplit{ws_waves});
    return found ? hipGetLastError() : hipErrorInvalidValue;
  });
  if (e != hipSuccess) return e;
  e = decode_chunks(dtype, q, k_pool, v_pool, block_table, kv_len, shared_len, group_size, ws_o, ws_ml, B, Hq, Hkv, D,
                    cap, page, n_pages, scale, s);
  if (e != hipSuccess) return e;
  return pra_attn_decode_combine(dtype, ws_o, ws_ml, kv_len, o, lse, B, Hq, D, cap, NC, s);
}
