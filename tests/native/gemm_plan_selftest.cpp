// The tail plan of the hand-written GEMMs (csrc/kernels/gemm_plan.h) on the CPU. Plain host C++, no GPU.
//   gemm_plan_selftest             reads lines "kind M N K cus" (kind: nt | wgrad) from stdin and prints
//                                  one line of key=value words per input line
//   gemm_plan_selftest exhaustive  compares the plan with a transcription of the launchers' expressions
//                                  before the plan existed, over tiles 1..2048, cus {64, 256, 304} and
//                                  K {32, 64, 96, 128, 4096}, both kinds; prints the count, exits 1 on a
//                                  difference
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "kernels/gemm_plan.h"

namespace {

// --- what pra_gemm_nt / pra_wgrad_gemm computed in place, with ws and tickets handed in ---------------
int old_tail_split(int nwg, int cus, int nk, int smax) {
  if (nwg <= cus || nwg % cus == 0) return 1;
  const int R = nwg % cus;
  double best = 1.0;
  int S = 1;
  for (int c = 2; c <= smax && c <= 8 && c <= nk; ++c) {
    const double t = (double)((R * c + cus - 1) / cus) / c;
    if (t < best - 1e-9) best = t, S = c;
  }
  return S;
}
struct Old {
  int nwg, kb, S, n_split, grid;
};
Old old_launch(bool nt, int M, int N, int K, int cus) {
  Old o;
  o.nwg = (M / 256) * (N / 256);
  o.kb = nt && K % 64 == 0 ? 64 : 32;  // KBx; the weight gradient: BK
  const int Ssplit = old_tail_split(o.nwg, cus, K / o.kb, 2);
  o.n_split = Ssplit > 1 ? o.nwg % cus : 0;
  o.S = o.n_split ? Ssplit : 1;
  o.grid = o.nwg - o.n_split + o.n_split * o.S;
  return o;
}

int exhaustive() {
  const int cuss[] = {64, 256, 304}, Ks[] = {32, 64, 96, 128, 4096};
  long n = 0;
  for (int kind = 0; kind < 2; ++kind)
    for (int cus : cuss)
      for (int K : Ks)
        for (int tiles = 1; tiles <= 2048; ++tiles) {
          // both factorisations of the tile count that every count has
          const int Ms[] = {256, 256 * tiles}, Ns[] = {256 * tiles, 256};
          for (int f = 0; f < 2; ++f) {
            const pra::GemmPlan p = pra::gemm_plan(kind, Ms[f], Ns[f], K, cus);
            const Old o = old_launch(kind == pra::kGemmNT, Ms[f], Ns[f], K, cus);
            const long ws = (long)o.n_split * o.S * 256 * 256;
            const bool same = p.tiles == o.nwg && p.kb == o.kb && p.S == o.S && p.n_split == o.n_split &&
                              p.grid == o.grid && p.ws_floats == ws && p.tickets == o.n_split;
            const pra::GemmPlan u = pra::gemm_unsplit(p);  // no scratch handed in
            const bool unsplit =
                u.tiles == o.nwg && u.kb == o.kb && u.S == 1 && !u.n_split && u.grid == o.nwg && !u.ws_floats && !u.tickets;
            if (!same || !unsplit) {
              printf("differs: kind=%d M=%d N=%d K=%d cus=%d\n", kind, Ms[f], Ns[f], K, cus);
              return 1;
            }
            ++n;
          }
        }
  printf("compared=%ld\n", n);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "exhaustive")) return exhaustive();
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty() || line[0] == '#') continue;
    std::istringstream in(line);
    std::string kind;
    int M = 0, N = 0, K = 0, cus = 0;
    if (!(in >> kind >> M >> N >> K >> cus) || (kind != "nt" && kind != "wgrad") || M <= 0 || N <= 0 || K <= 0 ||
        M % 256 || N % 256 || K % 32 || cus <= 0) {
      fprintf(stderr, "bad line: %s\n", line.c_str());
      return 2;
    }
    const pra::GemmPlan p = pra::gemm_plan(kind == "nt" ? pra::kGemmNT : pra::kGemmWgrad, M, N, K, cus);
    printf("tiles=%d kb=%d R=%d S=%d n_split=%d grid=%d ws=%ld tickets=%d\n", p.tiles, p.kb, p.tiles % cus, p.S,
           p.n_split, p.grid, p.ws_floats, p.tickets);
  }
  return 0;
}
