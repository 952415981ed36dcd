// What the paged-cache translation units share (attention_paged.hip, attention_decode_shared.hip): the
// table-entry idioms, the pool checks of the launchers and the effective shared length of a sequence group.
#pragma once
#include "common.h"
#include "launchers.h"

namespace pra {
namespace paged {

constexpr int kKC = 256;  // attention_decode.hip's chunk (pra_attn_decode_chunk; checked by the launchers)
constexpr float kNoMax = -1e30f;  // "no score yet" running max, as in the dense kernels

// c ? x : y on values, as mask arithmetic: a ?: over table entries invites the compiler to select between their
// addresses and load afterwards, which parks the entries in scratch memory
__device__ __forceinline__ int sel(bool c, int x, int y) {
  const int m = -(int)c;
  return (x & m) | (y & ~m);
}

// entry i of a small workgroup-uniform array, i uniform: a chain of scalar selects, no indexed register file
template <int N>
__device__ __forceinline__ int pick(const int (&e)[N], int i) {
  int r = e[0];
#pragma unroll
  for (int k = 1; k < N; ++k) r = sel(i == k, e[k], r);
  return r;
}

__device__ __forceinline__ bool mapped(int e, int n_pages) { return (unsigned)e < (unsigned)n_pages; }

// Whether the chunk at key c0 (a multiple of kKC) of group g (sequences g * n .. g * n + n - 1) belongs to the
// shared-prefix decode kernel: c0 < s_eff(g), where
//   s_eff(g) = floor(min(shared_len[g], cap, min_i clamp(kv_len[g n + i], 0, cap)) / kKC) * kKC
// counts the leading keys that every member's table row names alike and that every member attends to, in whole
// chunks. c0 < s_eff(g) holds exactly when each of those terms is at least c0 + kKC, so the lanes test one member
// each and vote: no reduction of values, and every load's address comes from the arguments alone (the early
// exit of a workgroup is two load latencies long). Wave-uniform, from device data alone; called by all 64 lanes.
__device__ __forceinline__ bool shared_prefix_covers(const int* __restrict__ shared_len,
                                                     const int* __restrict__ kv_len, int g, int n, int cap, int c0) {
  const int need = c0 + kKC;
  bool ok = min(shared_len[g], cap) >= need;
  for (int i = threadIdx.x & 63; i < n; i += 64) ok = (kv_len[(long)g * n + i] >= need) & ok;
  return __all(ok);
}

// log2(page) for the page sizes served, -1 otherwise
inline int page_shift(int page) { return page == 64 ? 6 : page == 128 ? 7 : page == 256 ? 8 : -1; }

// what every launcher checks of the pool and the table; P = ceil(cap / page)
inline bool pool_ok(const void* kp, const void* vp, const int* bt, int cap, int page, int n_pages) {
  return kp != nullptr && vp != nullptr && bt != nullptr && cap > 0 && page_shift(page) >= 0 && n_pages >= 1 &&
         (long)n_pages * page <= 0x7fffffffL;
}

// attention_paged.hip: the chunk launch of pra_attn_decode_paged (which has checked the shape). With shared_len
// it is the per-sequence remainder of pra_attn_decode_shared_paged: a chunk below the effective shared length
// of the sequence's group (of group_size members) is left to the shared kernel and writes nothing.
hipError_t decode_chunks(int dtype, const void* q, const void* k_pool, const void* v_pool, const int* block_table,
                         const int* kv_len, const int* shared_len, int group_size, float* ws_o, float* ws_ml, int B,
                         int Hq, int Hkv, int D, int cap, int page, int n_pages, float scale, hipStream_t s);

}  // namespace paged
}  // namespace pra
