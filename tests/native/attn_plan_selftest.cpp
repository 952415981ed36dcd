// Prints the attention launch plan (csrc/kernels/attn_plan.h) for each line of stdin. A line is a list of
// key=value words: the options of pra_attn_options (left out: the C++ default), the shape B S Hq Hkv D
// causal (default 1) skv (default S) fam (0 = bf16 / fp16, 1 = fp32, 2 = docs), window (0 / 1: a mid_event
// is handed in) and cus. Output: one line of key=value words per input line. Plain host C++, no GPU.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "kernels/attn_plan.h"

using namespace pra::attn;

int main() {
  static const char* const kDkdv[] = {"lds", "kreg", "ring", "p2"};
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty() || line[0] == '#') continue;
    pra_attn_options op;
    Shape s = {kFam16, 0, 0, 0, 0, 0, -1, true};
    int window = 0, cus = 256;
    std::istringstream in(line);
    std::string word;
    while (in >> word) {
      const size_t eq = word.find('=');
      if (eq == std::string::npos) {
        fprintf(stderr, "bad word %s\n", word.c_str());
        return 2;
      }
      const std::string key = word.substr(0, eq);
      const double val = atof(word.c_str() + eq + 1);
      const int iv = (int)val;
      struct { const char* name; int* p; } const ints[] = {
          {"fwd_pipe", &op.fwd_pipe},     {"dkdv_impl", &op.dkdv_impl},   {"dq_pipe", &op.dq_pipe},
          {"dkdv_split", &op.dkdv_split}, {"dkdv_kreg", &op.dkdv_kreg},   {"bwd_fused", &op.bwd_fused},
          {"bwd_window", &op.bwd_window}, {"fwd_order", &op.fwd_order},   {"dq_order", &op.dq_order},
          {"dkdv_order", &op.dkdv_order}, {"B", &s.B},                    {"S", &s.S},
          {"Hq", &s.Hq},                  {"Hkv", &s.Hkv},                {"D", &s.D},
          {"skv", &s.skv},                {"window", &window},            {"cus", &cus}};
      bool found = false;
      for (const auto& e : ints)
        if (key == e.name) *e.p = iv, found = true;
      if (key == "fwd_thr") op.fwd_thr = (float)val, found = true;
      if (key == "causal") s.causal = iv != 0, found = true;
      if (key == "fam") s.fam = (Family)iv, found = true;
      if (!found) {
        fprintf(stderr, "unknown key %s\n", key.c_str());
        return 2;
      }
    }
    if (s.skv < 0) s.skv = s.S;
    if (s.B <= 0 || s.S <= 0 || s.Hq <= 0 || s.Hkv <= 0 || s.Hq % s.Hkv || cus <= 0) {
      fprintf(stderr, "bad shape in: %s\n", line.c_str());
      return 2;
    }
    const BwdPlan b = bwd_plan(op, s, window != 0, cus);
    if (s.fam == kFam16) {
      const FwdPlan f = fwd_plan(op, s);
      printf("fwd_pipe=%d fwd_thr=%g fwd_grp=%d ", (int)f.pipe, f.thr, f.grp);
    }
    printf("fused=%d nw=%d dq_pipe=%d win_early=%d dkdv=%s nsplit=%d gq=%d gk=%d delta=%ld rc=%ld part=%ld acc=%ld "
           "qend=%ld ws=%ld\n",
           (int)b.fused, b.nw, (int)b.dq_pipe, (int)b.win_early, kDkdv[b.dkdv], b.nsplit, b.gq, b.gk, b.delta, b.rc,
           b.part, b.acc, b.qend, b.ws_floats);
  }
  return 0;
}
