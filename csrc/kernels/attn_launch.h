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
