// Stateless stochastic rounding of fp32 values to bf16 / fp16 (train.py --stochastic-rounding).
//
// The 16 random bits of an element are a pure function of (seed, step, flat position, tensor), so
// the result does not depend on launch geometry, bucket, stream, rank or replay:
//   g = idx >> 3, lane = idx & 7 (idx: the element's int64 position in the flat buffer)
//   out = Philox4x32-10(counter = {g & 0xffffffff, g >> 32, step, stream}, key = {seed lo, seed hi})
//   r = (out[lane >> 1] >> (16 * (lane & 1))) & 0xffff
// stream: 0 parameters, 1 exp_avg, 2 exp_avg_sq. One Philox call serves the 8 elements of an aligned
// 16-byte chunk of one tensor. The key schedule is uniform per launch and stays in scalar registers;
// a call is 20 32x32 -> 64 multiplies and ~38 xor on the vector unit.
//
// Rounding x to the 16-bit type T: NaN, inf and |x| above T's largest finite value take the plain
// round-to-nearest cast. Otherwise lo = x truncated toward zero to T, hi = the next T value away from
// zero, tfrac = floor((|x| - |lo|) / (|hi| - |lo|) * 65536), and the result is hi when r < tfrac, else
// lo (x == lo gives tfrac = 0). Sign kept, -0 stays -0. Everything is done on the bits of x with
// integer operations, so no compiler flag can fold this rounding with the fp32 rounding before it.
// pyrecover_amd/optim/sr.py is the same rule in torch (the tests' oracle and the CPU path).
#pragma once
#include "common.h"

namespace pra {

// (The launch-uniform arguments of a stochastic-rounding launch are launchers.h's pra_sr_args.)
enum : uint32_t { kSrStreamP = 0, kSrStreamM = 1, kSrStreamV = 2 };

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                              uint32_t k1, uint32_t (&out)[4]) {
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0;
  out[1] = c1;
  out[2] = c2;
  out[3] = c3;
}

// The four random words of the chunk of 8 elements that holds flat position idx.
__device__ __forceinline__ void sr_chunk_bits(unsigned long long seed, long long idx, uint32_t step, uint32_t stream,
                                              uint32_t (&out)[4]) {
  const unsigned long long g = (unsigned long long)idx >> 3;
  philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), step, stream, (uint32_t)seed, (uint32_t)(seed >> 32), out);
}

// fp32 bits -> 16-bit storage bits of T with the 16 random bits r.
template <typename T>
__device__ __forceinline__ uint32_t sr_round16(float x, uint32_t r) {
  const uint32_t bits = __float_as_uint(x), a = bits & 0x7fffffffu;
  if constexpr (__is_same(T, __bf16)) {
    if (a > 0x7f7f0000u) return __builtin_bit_cast(uint16_t, (__bf16)x);  // NaN, inf, above bf16's max
    return (bits >> 16) + (r < (bits & 0xffffu) ? 1u : 0u);
  } else {
    if (a > 0x477fe000u) return __builtin_bit_cast(uint16_t, __float2half_rn(x));  // NaN, inf, > 65504
    const uint32_t sign = (bits >> 16) & 0x8000u, e = a >> 23;
    uint32_t lo, tfrac;
    if (e >= 113u) {  // |x| >= 2^-14: an fp16 normal; 13 fp32 mantissa bits are dropped
      lo = (a - (112u << 23)) >> 13;
      tfrac = (a & 0x1fffu) << 3;
    } else {  // fp16 subnormal range: |x| in units of 2^-40 = 2^-24 (fp16's subnormal step) / 65536
      const uint32_t mant = (a & 0x7fffffu) | (e ? 0x800000u : 0u), ee = e ? e : 1u;  // |x| = mant * 2^(ee - 150)
      const uint32_t y = ee >= 110u ? mant << (ee - 110u) : (110u - ee < 32u ? mant >> (110u - ee) : 0u);
      lo = y >> 16;
      tfrac = y & 0xffffu;
    }
    return sign | (lo + (r < tfrac ? 1u : 0u));  // lo + 1 carries into the exponent at a binade's end
  }
}

// 8 fp32 values of one aligned chunk -> 16 B of T, stochastically rounded with the chunk's words.
template <typename T>
__device__ __forceinline__ void sr_pack8(const float (&v)[8], const uint32_t (&rnd)[4], uint32_t (&w)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
    w[i] = sr_round16<T>(v[2 * i], rnd[i] & 0xffffu) | (sr_round16<T>(v[2 * i + 1], rnd[i] >> 16) << 16);
}

// One element at flat position idx (the tail of a launch).
template <typename T>
__device__ __forceinline__ uint16_t sr_round_at(float x, unsigned long long seed, long long idx, uint32_t step,
                                                uint32_t stream) {
  uint32_t rnd[4];
  sr_chunk_bits(seed, idx, step, stream, rnd);
  const uint32_t lane = (uint32_t)idx & 7u;
  return (uint16_t)sr_round16<T>(x, (rnd[lane >> 1] >> (16u * (lane & 1u))) & 0xffffu);
}

}  // namespace pra
