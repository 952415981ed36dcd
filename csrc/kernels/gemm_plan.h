// Work decomposition of the hand-written GEMMs (gemm_nt.hip, gemm_wgrad.hip) as pure host functions:
// (kind, M, N, K, CU count) -> tiles, k-stage depth, the split of the partial last round, grid, and the
// scratch the split needs. Plain C++, no HIP (tests/native/gemm_plan_selftest.cpp compiles it with g++).
// pra_gemm_scratch returns GemmPlan's sizes and the launchers use the same plan: nothing else computes
// either.
#pragma once

namespace pra {

enum GemmKind { kGemmNT = 0, kGemmWgrad = 1 };

constexpr int kGemmTile = 256;  // workgroup tile, M and N (gemm_common.h BM, BN)
// Largest K-split of a partial last round. Weight gradient: W2 at 4 was 11% slower
// (profiles/r4/wgrad_w2_tail_split_ab.log).
constexpr int kGemmSmax = 2;

// Split of the partial last round: the R = nwg % cus tail tiles are split S ways over K when that
// fills whole rounds better (S <= smax, ties -> the smaller S). nk: k-stages of the kernel that runs.
// Returns S (1 = unsplit).
inline int gemm_tail_split(int nwg, int cus, int nk, int smax) {
  if (nwg <= cus || nwg % cus == 0) return 1;
  const int R = nwg % cus;
  double best = 1.0;  // unsplit: one more round
  int S = 1;
  for (int c = 2; c <= smax && c <= 8 && c <= nk; ++c) {
    const double t = (double)((R * c + cus - 1) / cus) / c;
    if (t < best - 1e-9) best = t, S = c;
  }
  return S;
}

struct GemmPlan {
  int tiles;       // 256 x 256 output tiles
  int kb;          // k depth of one LDS stage: NT 64 when K % 64 == 0 (two-buffer loop), else 32 (ring)
  int S;           // split of the tail tiles over K (1 = unsplit)
  int n_split;     // tail tiles that are split (0 when S == 1)
  int grid;        // tiles - n_split whole tiles, then n_split * S split units
  long ws_floats;  // fp32 partial tiles [n_split][S][256 * 256]
  int tickets;     // one int32 arrival counter per split tile
};

// The plan without a split tail: what runs when the caller has no scratch (the tail is then a partial
// data-parallel round).
inline GemmPlan gemm_unsplit(GemmPlan p) {
  p.S = 1;
  p.n_split = 0;
  p.grid = p.tiles;
  p.ws_floats = 0;
  p.tickets = 0;
  return p;
}

// M, N % 256 == 0, K % 32 == 0, cus > 0 (the launchers check)
inline GemmPlan gemm_plan(int kind, int M, int N, int K, int cus) {
  GemmPlan p;
  p.tiles = (M / kGemmTile) * (N / kGemmTile);
  p.kb = kind == kGemmNT && K % 64 == 0 ? 64 : 32;
  p.S = gemm_tail_split(p.tiles, cus, K / p.kb, kGemmSmax);
  if (p.S == 1) return gemm_unsplit(p);
  p.n_split = p.tiles % cus;
  p.grid = p.tiles - p.n_split + p.n_split * p.S;
  p.ws_floats = (long)p.n_split * p.S * kGemmTile * kGemmTile;
  p.tickets = p.n_split;
  return p;
}

}  // namespace pra
