// Kernel selection of attn_extend (attention_extend.hip / attention_extend_split.hip) as a pure host
// function: shape + CU count -> single pass or key split, the split's wave layout, grid and workspace.
// Plain C++, no HIP. Never device data: the choice is a function of (B, T, Hq, Hkv, D, cap, cus) alone.
#pragma once

typedef struct pra_attn_extend_plan_t {
  int split;       // 1: extend_split_kernel + extend_combine_kernel, 0: extend_fwd_kernel
  int ws_waves;    // split: waves that share a 32-row sub-tile and divide a chunk's key tiles (4, 2 or 1)
  int chunks;      // split: key chunks of the cache, ceil(cap / kExtendChunk)
  long blocks;     // workgroups of the (first) kernel
  long ws_floats;  // fp32 words of workspace (0 on the single pass)
} pra_attn_extend_plan_t;

namespace pra {
namespace attn {

// Keys per chunk of the split; a multiple of 256 (four 64-key tiles for each of four waves). Chunk
// boundaries are a function of the key position alone. Chosen by measurement (profiles/decode/README.md).
constexpr int kExtendChunk = 512;
static_assert(kExtendChunk % 256 == 0, "chunk length");

inline int extend_ws_waves(long R) { return R <= 32 ? 4 : R <= 64 ? 2 : 1; }

// fp32 words of the split's workspace: partial outputs [B][T][Hq][NC][D], then (max, sum) [B][T][Hq][NC][2]
inline long extend_ws_floats(int B, int T, int Hq, int D, int cap) {
  const long NC = (cap + kExtendChunk - 1) / kExtendChunk;
  return (long)B * T * Hq * NC * (D + 2);
}

// split: -1 by shape, 0 single pass, 1 key split (honoured for any shape, one chunk included).
// By shape the split runs when the single pass would leave at least half of the CUs without a block
// (2 blocks1 <= cus) and the cache has at least 4 chunks: below that the partials and the second
// launch cost more than the idle CUs (and every cache of up to 3 chunks keeps the single pass's bits).
inline pra_attn_extend_plan_t extend_plan(int B, int T, int Hq, int Hkv, int D, int cap, int cus, int split) {
  const long R = (long)T * (Hq / Hkv);
  const long blocks1 = (R + 127) / 128 * Hkv * B;
  const int NC = (cap + kExtendChunk - 1) / kExtendChunk;
  const bool on = split > 0 || (split < 0 && NC >= 4 && 2 * blocks1 <= cus);
  if (!on) return {0, 1, 1, blocks1, 0};
  const int ws = extend_ws_waves(R);
  const long rows = 128 / ws;  // rows of a block
  return {1, ws, NC, (R + rows - 1) / rows * Hkv * B * NC, extend_ws_floats(B, T, Hq, D, cap)};
}

}  // namespace attn
}  // namespace pra
