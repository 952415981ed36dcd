// Internal to the training-attention translation units: the launch functions behind pra_attn_fwd /
// pra_attn_bwd (attention.hip routes to them) and the host helpers they share. Kernels still take
// scalars and __restrict__ pointers one by one: never the block (profiles/adamw_args/README.md).
#pragma once
#include "common.h"
#include "launchers.h"

namespace pra {
namespace attn {

hipError_t docs_fwd(const pra_attn_args& a, hipStream_t st);                     // attention_docs.hip
hipError_t docs_bwd(const pra_attn_args& a, const BwdPlan& pl, hipStream_t st);
hipError_t f32_fwd(const pra_attn_args& a, hipStream_t st);                      // attention_f32.hip
hipError_t f32_bwd(const pra_attn_args& a, hipStream_t st);
hipError_t fused_bwd(const pra_attn_args& a, const BwdPlan& pl, hipStream_t st);  // attention_bwd_fused.hip
// attention_extend_split.hip: the key-split arm of pra_attn_extend (which has checked the shape)
hipError_t extend_split(int dtype, const void* q, long ldq, const void* k_cache, const void* v_cache,
                        const int* kv_len, void* o, float* lse, float* ws, int B, int T, int Hq, int Hkv, int D,
                        int cap, const pra_attn_extend_plan_t& pl, float scale_log2, hipStream_t s);

// CUs of the current device (256 when it cannot be asked): what the plans take as `cus`
inline int device_cus() {
  static int cus[64] = {0};
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= 64) return 256;
  if (cus[d] == 0 && (hipDeviceGetAttribute(&cus[d], hipDeviceAttributeMultiprocessorCount, d) != hipSuccess || cus[d] <= 0))
    cus[d] = 256;
  return cus[d];
}

inline Shape shape_of(const pra_attn_args& a) {
  const Family fam = a.doc_start != nullptr ? kFamDocs : a.dtype == kF32 ? kFamF32 : kFam16;
  return {fam, a.B, a.S, a.Hq, a.Hkv, a.D, a.skv, a.causal != 0};
}

// token strides in elements, multiples of m (16-B vector accesses: 8 for 16-bit, 4 for fp32)
inline bool strides_ok(const pra_attn_args& a, bool bwd, int m) {
  if (a.ldq % m || a.ldk % m || a.ldv % m || a.ldo % m) return false;
  return !bwd || !(a.lddo % m || a.lddq % m || a.lddk % m || a.lddv % m);
}

// f(T{}) for the 16-bit element type of `dtype`. The standalone harness (tools/attn_variants.sh)
// builds the bf16 instantiations only.
template <class F>
inline hipError_t dispatch_16bit(int dtype, F&& f) {
  if (dtype == kBF16) return f(__bf16{});
#if !PRA_ATTN_HARNESS
  if (dtype == kF16) return f(_Float16{});
#endif
  return hipErrorInvalidValue;
}

// The value lists of dispatch (common.h). They ascend: instantiations then come out in the order the
// kernels have always had in the code object (D 128 before 64, causal before full, 8 waves before 4).
using HeadDim = One<64, 128>;
using Causal = One<0, 1>;
using Waves = One<4, 8>;  // BwdPlan::nw

}  // namespace attn
}  // namespace pra
