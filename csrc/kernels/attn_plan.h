// Kernel selection of the training attention as pure host functions: options + shape + window + CU count
// -> which kernels run, their grid order, and where each finds its share of the fp32 workspace. Plain
// C++, no HIP (tests/native/attn_plan_selftest.cpp compiles it with g++). pra_attn_bwd_workspace returns
// BwdPlan::ws_floats and the launches use BwdPlan's offsets: nothing else computes either.
#pragma once

// Kernel selection knobs, set through pra_attn_set_options (pyrecover_amd._ext); no environment is read.
typedef struct pra_attn_options {
  // forward: -1 = by shape (pipelined fwd_p_kernel for causal, fwd_kernel for full attention),
  // 0 = fwd_kernel, 1 = fwd_p_kernel (a 16x16x32 forward of fwd_kernel's structure measured 0.766 vs
  // 0.727 ms for fwd_p_kernel, profiles/r5/attn/fwd16_vs_fwd.log, and was removed). The pipelined kernel's non-causal instantiation spills at
  // D = 128, and padded non-causal keys (skv < S) need fwd_kernel's key bound.
  // (B8 S2048 H32: 0.460 -> 0.422 ms; S8192 H32/8: 0.654 -> 0.615 ms with the pipelined kernel.)
  int fwd_pipe = -1;
  // Rescale threshold of the pipelined forward (cdna guide T13), log2 units: O and l are rescaled
  // only when some row's max grows by more than thr, so P stays below 2^thr (fp32 accumulators;
  // bf16 P keeps its relative precision). 0 = exact rescale at every growth.
  float fwd_thr = 8.f;
  // dK/dV: -1 = by shape (dkdv_use_p2), 0 = two-wave bwd_dkdv_kernel, 1 = pipelined bwd_dkdv_p2_kernel
  int dkdv_impl = -1;
  // dQ: -1/1 = region-pipelined bwd_dq_kernel<PIPE>, 0 = plain (padded non-causal keys: always plain)
  int dq_pipe = -1;
  // pipelined dK/dV kernel, query heads per block: 1 = all of the kv head's Hq / Hkv heads in one
  // block (default), n = Hq / Hkv / n heads per block plus an fp32 reduction, -1 = by grid size
  // (dkdv_split) when no side-stream job waits for the window. Not by default: it pays only without
  // the overlapped optimizer, and its fp32 partial sums would make the gradients depend on whether
  // the optimizer overlaps (tests/test_xgmi_gpu.py compares the two bitwise)
  int dkdv_split = 1;
  // two-wave dK/dV kernel (NW = 8, D = 128): 2 = ring-staged bwd_dkdv_r_kernel (K in registers,
  // Q/dO by LDS-DMA, one barrier per query tile; B16 S2048 H32 bwd 2.39 -> 2.27 ms,
  // profiles/r5/attn/harness_dkdv_ring.log), 1 = bwd_dkdv_kernel with K fragments held in registers
  // (KREG), 0 = bwd_dkdv_kernel reading K from LDS, -1 = KREG unless a side-stream job waits for the
  // dK/dV window (below) (r4: KREG 2.387 -> 2.358 ms alone, but 1058.0 vs 1055.5 ms in the 7B step:
  // profiles/r4/attn_ab_dkdv_kreg_b16.log, step_ab_7b_b16_kreg.log), -2 (default) = the ring kernel
  // unless a side-stream job waits for the window, else 0: the ring kernel's 242 VGPRs leave no
  // room on the SIMDs for the overlapped AdamW waves (the LDS kernel's 215 do), so in the overlapped
  // 7B B16 step it is not faster (1054.7 vs 1053.3 ms, profiles/r5/step_ab_ring.log)
  int dkdv_kreg = -2;
  // fused backward (attention_bwd_fused.hip: dQ, dK, dV in one workgroup per (batch, kv head)):
  // -1 = by shape (use_fused), 0 = never (split dQ + dK/dV kernels; the default), 1 = whenever
  // it applies. Not the default: alone it is faster (7B B16 step without the AdamW update 1032.7 ->
  // 1025.7 ms), but its 256-VGPR waves leave no room for the overlapped update's waves, which the split
  // dK/dV kernel hosts (with the update 1045.4 vs 1048.3 ms; profiles/r5/attn_fused/). The choice must
  // not depend on the window (dQ differs in the last bits), so it is a run-wide setting.
  int bwd_fused = 0;
  // where the side-stream window (mid_event) opens in the split backward: 0 = between the dQ and
  // the dK/dV kernels, 1 = before the dQ kernel (the update then runs beside both), -1 (default) = by
  // shape (window_before_dq): before dQ at <= 4096 tokens per call, where the dK/dV kernel alone is
  // too short a window (same-process A/B: Llama-3-8B B1 S2048 110.06 -> 109.61 ms, 7B B1 98.62 ->
  // 97.96 ms; at 8192 tokens slower: 8B S8192 B1 +2.35%, 8B S2048 B4 +0.33%, 7B B16 +0.5%;
  // profiles/r5/window/). Bitwise neutral: only the event moves.
  int bwd_window = -1;
  // block order of the pipelined forward (block_tile): 0 = heavy query tiles first across the grid,
  // G > 0 = XCD-grouped, G heads per group; -1 = by shape (attn_grp)
  int fwd_order = 0;
  int dq_order = 0;    // the same for the dQ kernel
  int dkdv_order = 0;  // and the two-wave / ring dK/dV kernels (key tiles, lightest last)
  // (A higher s_setprio for the backward kernels' waves than the overlapped AdamW update's, 1 or 3,
  // dK/dV and dQ: neutral in the 7B B16 step, 1058.0 / 1058.2 vs 1058.0 ms; profiles/r6/
  // step_ab_7b_b16_bwd_prio.log. Removed.)
} pra_attn_options;

namespace pra {
namespace attn {

constexpr float kLog2e = 1.4426950408889634f;

enum Family { kFam16 = 0, kFamF32 = 1, kFamDocs = 2 };  // bf16 / fp16, fp32, document-masked 16-bit
struct Shape {
  Family fam;
  int B, S, Hq, Hkv, D;
  int skv;  // real length of a zero-padded sequence (S otherwise)
  bool causal;
};

struct FwdPlan {  // kFam16 only: the fp32 and docs forwards have one kernel each
  bool pipe;      // fwd_p_kernel, else fwd_kernel
  float thr;
  int grp;        // block_tile group size
};

enum DkDv { kDkdvLds = 0, kDkdvKreg = 1, kDkdvRing = 2, kDkdvP2 = 3 };
struct BwdPlan {
  bool fused;      // bwd_rowc_kernel + bwd_fused_kernel; of the fields below only rc, acc and ws_floats hold
  int nw;          // waves per block of the dQ and two-wave dK/dV kernels: 8, or 4 when S % 256
  bool dq_pipe;    // bwd_dq_kernel<PIPE>
  bool win_early;  // mid_event before the dQ kernel, else between dQ and dK/dV
  DkDv dkdv;
  int nsplit;      // p2: query-head splits (> 1: fp32 partials + dkdv_reduce_kernel)
  int gq, gk;      // block_tile group sizes of the dQ and the two-wave / ring dK/dV grids
  // offsets into the workspace, in floats; -1 = that kernel takes a null pointer
  long delta;      // [B Hq S] rowsum(dO * O)
  long rc;         // [2][B Hq S] row constants (-lse / scale, -delta): ring, p2 and the fused kernel
  long part;       // p2 split partials [nsplit][2][B S Hkv D]
  long acc;        // fused: dQ partials [B Hq S D], then 1024 floats of scratch per workgroup
  long qend;       // docs: the dK/dV query-loop ends (int32) [B S / 128]
  long ws_floats;  // total; does not depend on the window (callers allocate before they know it)
};

inline bool window_before_dq(const pra_attn_options& op, int B, int S) {
  const int w = op.bwd_window;
  return w == 1 || (w < 0 && (long)B * S <= 4096);
}

// Heads per XCD group for an nqt x BH grid under option `order`, 0 when the grid does not split.
// By shape (order < 0): at least the rep = Hq / Hkv query heads that share a kv head (forward and dQ
// grids; 1 for the dK/dV grids, whose heads are kv heads), and at least 32 blocks (one per CU of
// an XCD) per group. B16 S2048 H32 D128 causal (harness, profiles/r5/attn_order/): forward
// 0.740 -> 0.650 ms, dQ + dK/dV 2.31 -> 2.11 ms; B1 S8192 H32/8 forward 0.508 -> 0.499 ms.
inline int attn_grp(int order, int nqt, int BH, int rep) {
  if (order == 0 || BH % 8) return 0;
  int g = order > 0 ? order : 1;
  if (order < 0)
    while ((g * 2 <= rep || g * 2 * nqt <= 32) && (BH / 8) % (g * 2) == 0) g *= 2;
  return (BH / 8) % g == 0 ? g : 0;
}

// dK/dV kernel choice. D = 64: 64 KB of LDS and <= 256 VGPRs, so two pipelined one-wave blocks share
// a CU and hide each other's prologue (B16 S2048 H16: 0.74 -> 0.68 ms bwd). At D = 128 the pipelined
// kernel wins only while the two-wave kernel's grid ((S/256) Hkv B blocks, one per CU) is at most one
// round of the chip's 256 CUs, where its causal work imbalance is exposed: S 8192 GQA 32/8 bwd B1
// 2.56 -> 1.98 ms with p2, but B4 7.30 (two-wave) vs 7.89 ms (p2) (profiles/attn_dkdv_select_r2.log).
inline bool dkdv_use_p2(const pra_attn_options& op, const Shape& s) {
  const int impl = op.dkdv_impl;
  const long grid2 = (long)(s.S / 256) * s.Hkv * s.B;
  return impl == 1 || (impl < 0 && (s.D == 64 || ((long)(s.Hq / s.Hkv) * s.S >= 8192 && grid2 <= 256)));
}

// Window rule (dkdv_split / dkdv_kreg = -1): when the caller hands a mid_event, a side-stream job
// (the overlapped AdamW update, ops/sched.py) runs beside the dK/dV kernel, and a shorter kernel only
// pushes the rest of that job onto the GEMMs after it. In the step, the faster variants then lose:
// Llama-3-8B B1 S2048 109.1 ms split vs 108.3 unsplit (eager update: 109.7 vs 113.6), 7B B16
// 1058.0 KREG vs 1055.5 (profiles/r4/step_ab_*_split_sched.log, *_kreg.log). So both apply only
// when no job waits for the window (e.g. gradient-accumulation micro-steps, no overlapped update).
//
// GQA at small batch: the pipelined dK/dV grid is (S / 128) Hkv B blocks, one per CU at D = 128
// (Llama-3-8B B1 S2048 bwd 0.297 -> 0.206 (2 splits) -> 0.172 ms (4); S8192: 1.717 ms unsplit, the
// best: profiles/r4/attn_ab_dkdv_split_*.log)
// -- 128 blocks (half the chip) for Llama-3-8B B1 S2048 H32/8, and the causal work per block falls
// 16:1 from the first key block to the last. Splitting the kv head's query heads over n blocks gives
// n times the grid; with the heavy key blocks dispatched first, a CU that drew a light block picks
// up the next one, so two rounds of blocks even out to ~ (S/128 + 1) / 2 steps of work per CU. The
// price is an fp32 partial per split and one reduction pass (2 n B S Hkv D floats).
inline int dkdv_split(const pra_attn_options& op, const Shape& s) {
  const int nrep = s.Hq / s.Hkv;
  int n = op.dkdv_split;
  if (n < 0) {
    const long grid = (long)(s.S / 128) * s.Hkv * s.B, want = s.D == 64 ? 1024 : 512;
    n = 1;
    while (grid * n < want && nrep % (2 * n) == 0) n *= 2;
  }
  return (n >= 1 && nrep % n == 0) ? n : 1;
}

// Fused backward (attention_bwd_fused.hip) applies at D = 128, S % 256 == 0 without key padding. By
// shape it runs when its grid -- one workgroup per (batch, kv head), each walking all S / 256 key
// blocks -- fills whole rounds of the chip (>= 90% of the slots of its last round busy): 7B-class MHA
// at batch >= 8. Its choice never depends on the AdamW window (mid_event), so overlapped and plain
// optimizer steps see the same gradients.
inline bool fused_shape_ok(int S, int D) { return D == 128 && S % 256 == 0; }
inline bool use_fused(const pra_attn_options& op, const Shape& s, long cus) {
  const int mode = op.bwd_fused;
  if (mode == 0 || !fused_shape_ok(s.S, s.D) || s.skv != s.S) return false;
  if (mode == 1) return true;
  const long grid = (long)s.B * s.Hkv;
  const long rounds = (grid + cus - 1) / cus;
  return grid >= cus && grid * 10 >= rounds * cus * 9;
}

inline FwdPlan fwd_plan(const pra_attn_options& op, const Shape& s) {
  FwdPlan p;
  p.pipe = (s.causal || s.skv >= s.S) && (op.fwd_pipe >= 0 ? op.fwd_pipe != 0 : s.causal);
  p.thr = op.fwd_thr;
  p.grp = attn_grp(op.fwd_order, (s.S + 255) / 256, s.Hq * s.B, s.Hq / s.Hkv);
  return p;
}

// window: the caller hands a mid_event (a side-stream job waits for the dK/dV window); cus: CUs of the device
inline BwdPlan bwd_plan(const pra_attn_options& op, const Shape& s, bool window, int cus) {
  BwdPlan p = {false, 8, false, false, kDkdvLds, 1, 0, 0, 0, -1, -1, -1, -1, 0};
  const long nrc = (long)s.B * s.Hq * s.S;
  if (s.fam == kFamF32) {  // delta only; the 3 nrc are what the entry point has always asked for
    p.ws_floats = 3 * nrc;
    return p;
  }
  if (s.fam == kFamDocs) {
    p.qend = nrc;
    p.ws_floats = nrc + (long)s.B * (s.S / 128);
    return p;
  }
  const bool p2 = dkdv_use_p2(op, s);
  const int nsplit = p2 ? dkdv_split(op, s) : 1;
  // split kernels or fused (row constants at nrc as well): sized for either, whatever the window says
  const long split = 3 * nrc + (nsplit > 1 ? 2L * nsplit * s.B * s.S * s.Hkv * s.D : 0);
  const long fused =
      op.bwd_fused != 0 && fused_shape_ok(s.S, s.D) ? 3 * nrc + nrc * s.D + 1024L * s.B * s.Hkv : 0;
  p.ws_floats = split > fused ? split : fused;
  if (use_fused(op, s, cus)) {
    p.fused = true;
    p.rc = nrc;
    p.acc = 3 * nrc;
    return p;
  }
  // 8-wave (256-row) blocks; S % 256 != 0 (S % 128 == 0) takes the 4-wave instantiations
  p.nw = s.S % 256 ? 4 : 8;
  // the pipelined dQ kernel has no key bound: padded non-causal sequences take the plain one
  p.dq_pipe = (s.causal || s.skv >= s.S) && op.dq_pipe != 0;
  p.win_early = window_before_dq(op, s.B, s.S);
  const bool big = p.nw == 8 && s.D == 128;  // bwd_dkdv_r_kernel and KREG exist only there
  if (p2) {
    p.dkdv = kDkdvP2;
    p.nsplit = window && op.dkdv_split < 0 ? 1 : nsplit;
  } else if (big && (op.dkdv_kreg == 2 || (op.dkdv_kreg == -2 && !window))) {
    p.dkdv = kDkdvRing;
  } else if (big && (op.dkdv_kreg == 1 || (op.dkdv_kreg < 0 && !window))) {
    p.dkdv = kDkdvKreg;
  }
  const int nqt = s.S / (32 * p.nw);
  p.gq = attn_grp(op.dq_order, nqt, s.Hq * s.B, s.Hq / s.Hkv);
  p.gk = p2 ? 0 : attn_grp(op.dkdv_order, nqt, s.Hkv * s.B, 1);
  // the dQ kernel writes the row constants only when a dK/dV kernel reads them
  p.rc = p2 || p.dkdv == kDkdvRing ? nrc : -1;
  p.part = p.nsplit > 1 ? 3 * nrc : -1;
  return p;
}

}  // namespace attn
}  // namespace pra
