// Fused causal-LM cross-entropy over bf16/fp16/fp32 logits (reference train.py:263-266:
// `cross_entropy(logits.float(), labels, reduction="sum") / labels.ne(-100).sum()`).
// A label outside [0, V) is treated exactly like `ignore_index` by all three kernels (label_valid):
// loss 0, not counted in n_valid, zero gradient row.
//
// Forward: one 256-thread block per row, a single streaming pass with an online
// (max, sum-exp) pair per lane -> per-row log-sum-exp and loss, no fp32 copy of the logits.
// A single-block kernel then sums the row losses in a fixed order and divides by the
// number of non-ignored labels, all on device (no host sync for `n_items`).
// Backward: d logits = (softmax - onehot) * grad_out / n_items, written IN PLACE over the
// logits (they are dead after the backward), so the [T, V] activation is never duplicated.
#include "common.h"

namespace pra {

__device__ __forceinline__ bool label_valid(long lab, long V, long ignore_index) {
  return lab != ignore_index && lab >= 0 && lab < V;
}

template <typename T>
__global__ __launch_bounds__(256) void xent_fwd_kernel(const T* __restrict__ logits, const int64_t* __restrict__ labels,
                                                       float* __restrict__ lse_out, float* __restrict__ loss_row,
                                                       long V, long ld, long ignore_index) {
  __shared__ float sm[4], ss[4];
  const long row = blockIdx.x;
  const T* x = logits + row * ld;
  const int tid = threadIdx.x;
  float m = -INFINITY, s = 0.f;
  const long V8 = (V / 8) * 8;
  for (long c = (long)tid * 8; c < V8; c += 2048) {
    float v[8];
    load8<T>(x + c, v);
    float lm = v[0];
#pragma unroll
    for (int j = 1; j < 8; ++j) lm = fmaxf(lm, v[j]);
    const float nm = fmaxf(m, lm);
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc += __expf(v[j] - nm);
    s = s * __expf(m - nm) + acc;
    m = nm;
  }
  for (long c = V8 + tid; c < V; c += 256) {  // tail (V not a multiple of 8)
    const float v = to_f<T>(x[c]);
    const float nm = fmaxf(m, v);
    s = s * __expf(m - nm) + __expf(v - nm);
    m = nm;
  }
  // combine (m, s) across the wave then the block
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(m, o, 64), os = __shfl_xor(s, o, 64);
    const float nm = fmaxf(m, om);
    s = (m == -INFINITY ? 0.f : s * __expf(m - nm)) + (om == -INFINITY ? 0.f : os * __expf(om - nm));
    m = nm;
  }
  if ((tid & 63) == 0) { sm[tid >> 6] = m; ss[tid >> 6] = s; }
  __syncthreads();
  if (tid == 0) {
    float M = sm[0];
    for (int i = 1; i < 4; ++i) M = fmaxf(M, sm[i]);
    float S = 0.f;
    for (int i = 0; i < 4; ++i) S += (sm[i] == -INFINITY ? 0.f : ss[i] * __expf(sm[i] - M));
    const float lse = M + __logf(S);
    lse_out[row] = lse;
    const long lab = labels[row];
    loss_row[row] = label_valid(lab, V, ignore_index) ? lse - to_f<T>(x[lab]) : 0.f;
  }
}

// out[0] = sum(loss_row) / n_valid ; out[1] = n_valid (as float). One block, fixed order.
__global__ __launch_bounds__(256) void xent_reduce_kernel(const float* __restrict__ loss_row,
                                                          const int64_t* __restrict__ labels, float* __restrict__ out,
                                                          long T, long V, long ignore_index) {
  __shared__ float red[4];
  float s = 0.f, n = 0.f;
  for (long i = threadIdx.x; i < T; i += 256) {
    s += loss_row[i];
    n += label_valid(labels[i], V, ignore_index) ? 1.f : 0.f;
  }
  s = block_sum<4>(s, red);
  n = block_sum<4>(n, red);
  if (threadIdx.x == 0) {
    out[0] = s / n;
    out[1] = n;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void xent_bwd_kernel(T* __restrict__ logits, const int64_t* __restrict__ labels,
                                                       const float* __restrict__ lse, const float* __restrict__ stats,
                                                       const float* __restrict__ grad_out, long V, long ld,
                                                       long ignore_index) {
  const long row = blockIdx.x;
  T* x = logits + row * ld;
  const long lab = labels[row];
  const bool ign = !label_valid(lab, V, ignore_index);
  const float scale = ign ? 0.f : grad_out[0] / stats[1];
  const float l = lse[row];
  const long V8 = (V / 8) * 8;
  for (long c = (long)threadIdx.x * 8; c < V8; c += 2048) {
    float v[8];
    load8<T>(x + c, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (__expf(v[j] - l) - ((c + j) == lab ? 1.f : 0.f)) * scale;
    store8<T>(x + c, v);
  }
  for (long c = V8 + threadIdx.x; c < V; c += 256) {
    const float v = to_f<T>(x[c]);
    x[c] = from_f<T>((__expf(v - l) - (c == lab ? 1.f : 0.f)) * scale);
  }
}

// ---- regularised objective and logit telemetry (--z-loss, --label-smoothing, --logit-stats) ----
// Per valid row: nll = lse - x[label], smooth = lse - mean(x[:V]), zterm = z * lse^2;
// objective = ((1 - eps) * sum nll + eps * sum smooth + sum zterm) / n_valid.
// The plain kernels above stay as they are (the default path); at z = 0, eps = 0 these compute the
// same lse, objective, n_valid and dlogits bit for bit.

// The plain forward's pass with, for SMOOTH, an fp32 per-lane sum of the logits (columns < V only:
// the padding columns of a strided buffer never enter it), combined over the wave and the block in a
// fixed order. Writes lse[row] and the row's nll and smooth (0 for a row that is not valid; smooth is
// 0 everywhere without SMOOTH).
template <typename T, bool SMOOTH>
__global__ __launch_bounds__(256) void xent_fwd_reg_kernel(const T* __restrict__ logits,
                                                           const int64_t* __restrict__ labels,
                                                           float* __restrict__ lse_out, float* __restrict__ nll_row,
                                                           float* __restrict__ smooth_row, long V, long ld,
                                                           long ignore_index) {
  __shared__ float sm[4], ss[4], sx[4];
  const long row = blockIdx.x;
  const T* x = logits + row * ld;
  const int tid = threadIdx.x;
  float m = -INFINITY, s = 0.f, xs = 0.f;
  const long V8 = (V / 8) * 8;
  for (long c = (long)tid * 8; c < V8; c += 2048) {
    float v[8];
    load8<T>(x + c, v);
    float lm = v[0];
#pragma unroll
    for (int j = 1; j < 8; ++j) lm = fmaxf(lm, v[j]);
    const float nm = fmaxf(m, lm);
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc += __expf(v[j] - nm);
    s = s * __expf(m - nm) + acc;
    m = nm;
    if (SMOOTH) {
      float a8 = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) a8 += v[j];
      xs += a8;
    }
  }
  for (long c = V8 + tid; c < V; c += 256) {  // tail (V not a multiple of 8)
    const float v = to_f<T>(x[c]);
    const float nm = fmaxf(m, v);
    s = s * __expf(m - nm) + __expf(v - nm);
    m = nm;
    if (SMOOTH) xs += v;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(m, o, 64), os = __shfl_xor(s, o, 64);
    const float nm = fmaxf(m, om);
    s = (m == -INFINITY ? 0.f : s * __expf(m - nm)) + (om == -INFINITY ? 0.f : os * __expf(om - nm));
    m = nm;
  }
  if (SMOOTH) xs = wave_sum(xs);
  if ((tid & 63) == 0) {
    sm[tid >> 6] = m;
    ss[tid >> 6] = s;
    if (SMOOTH) sx[tid >> 6] = xs;
  }
  __syncthreads();
  if (tid == 0) {
    float M = sm[0];
    for (int i = 1; i < 4; ++i) M = fmaxf(M, sm[i]);
    float S = 0.f;
    for (int i = 0; i < 4; ++i) S += (sm[i] == -INFINITY ? 0.f : ss[i] * __expf(sm[i] - M));
    const float lse = M + __logf(S);
    lse_out[row] = lse;
    const long lab = labels[row];
    const bool ok = label_valid(lab, V, ignore_index);
    nll_row[row] = ok ? lse - to_f<T>(x[lab]) : 0.f;
    float sr = 0.f;
    if (SMOOTH && ok) {
      float X = 0.f;
      for (int i = 0; i < 4; ++i) X += sx[i];
      sr = lse - X / (float)V;
    }
    smooth_row[row] = sr;
  }
}

// stats[8] = {objective, n_valid, sum nll / n, z * sum lse^2 / n, sum smooth / n, mean lse, max |lse|, 0},
// lse over the valid rows only. One block, fixed order; no valid row: 0/0 = NaN, n = 0, max = 0.
// The row losses are summed in xent_reduce_kernel's order (256 threads, each its rows in sequence, then the
// wave and the block), so that the objective at z = 0, eps = 0 is the plain loss bit for bit; the loop is
// unrolled so that the loads of eight trips are in flight together (the block walks four arrays).
__global__ __launch_bounds__(256) void xent_reduce_reg_kernel(const float* __restrict__ nll_row,
                                                              const float* __restrict__ smooth_row,
                                                              const float* __restrict__ lse,
                                                              const int64_t* __restrict__ labels,
                                                              float* __restrict__ out, long T, long V,
                                                              long ignore_index, float z, float eps) {
  __shared__ float red[4];
  float s = 0.f, n = 0.f, sq = 0.f, sl = 0.f, sm = 0.f, mx = 0.f;
#pragma unroll 8
  for (long i = threadIdx.x; i < T; i += 256) {
    const bool ok = label_valid(labels[i], V, ignore_index);
    const float l = ok ? lse[i] : 0.f;
    s += nll_row[i];
    sm += smooth_row[i];
    n += ok ? 1.f : 0.f;
    sl += l;
    sq += l * l;
    mx = fmaxf(mx, fabsf(l));
  }
  s = block_sum<4>(s, red);
  n = block_sum<4>(n, red);
  sm = block_sum<4>(sm, red);
  sl = block_sum<4>(sl, red);
  sq = block_sum<4>(sq, red);
  mx = block_max<4>(mx, red);
  if (threadIdx.x == 0) {
    const float ce = s / n, zt = z * (sq / n), sv = sm / n;
    out[0] = (1.f - eps) * ce + eps * sv + zt;
    out[1] = n;
    out[2] = ce;
    out[3] = zt;
    out[4] = sv;
    out[5] = sl / n;
    out[6] = mx;
    out[7] = 0.f;
  }
}

// d logits = (softmax * (1 + 2 z lse) - (1 - eps) onehot - eps / V) * grad_out / n, in place, columns
// < V only. on = (1 - eps) + eps / V and off = eps / V come rounded from the host; at z = 0, eps = 0
// the factor is exactly 1.0f and the subtracted terms exactly 1 and 0: the plain kernel's values.
template <typename T>
__global__ __launch_bounds__(256) void xent_bwd_reg_kernel(T* __restrict__ logits, const int64_t* __restrict__ labels,
                                                           const float* __restrict__ lse,
                                                           const float* __restrict__ stats,
                                                           const float* __restrict__ grad_out, long V, long ld,
                                                           long ignore_index, float z, float on, float off) {
  const long row = blockIdx.x;
  T* x = logits + row * ld;
  const long lab = labels[row];
  const bool ign = !label_valid(lab, V, ignore_index);
  const float scale = ign ? 0.f : grad_out[0] / stats[1];
  const float l = lse[row];
  const float f = 1.f + 2.f * z * l;
  const long V8 = (V / 8) * 8;
  for (long c = (long)threadIdx.x * 8; c < V8; c += 2048) {
    float v[8];
    load8<T>(x + c, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (__expf(v[j] - l) * f - ((c + j) == lab ? on : off)) * scale;
    store8<T>(x + c, v);
  }
  for (long c = V8 + threadIdx.x; c < V; c += 256) {
    const float v = to_f<T>(x[c]);
    x[c] = from_f<T>((__expf(v - l) * f - (c == lab ? on : off)) * scale);
  }
}

}  // namespace pra

extern "C" {

// stats: float[2] device buffer -> {mean loss, n_valid}
hipError_t pra_xent_fwd(int dtype, const void* logits, const int64_t* labels, float* lse, float* loss_row,
                        float* stats, long T, long V, long ld, long ignore_index, hipStream_t s) {
  if (ld % 8) return hipErrorInvalidValue;
  PRA_DISPATCH_FLOAT(dtype, LT,
                     hipLaunchKernelGGL((pra::xent_fwd_kernel<LT>), dim3(T), dim3(256), 0, s, (const LT*)logits,
                                        labels, lse, loss_row, V, ld, ignore_index));
  hipLaunchKernelGGL(pra::xent_reduce_kernel, dim3(1), dim3(256), 0, s, loss_row, labels, stats, T, V, ignore_index);
  return hipGetLastError();
}

hipError_t pra_xent_bwd(int dtype, void* logits, const int64_t* labels, const float* lse, const float* stats,
                        const float* grad_out, long T, long V, long ld, long ignore_index, hipStream_t s) {
  if (ld % 8) return hipErrorInvalidValue;
  PRA_DISPATCH_FLOAT(dtype, LT,
                     hipLaunchKernelGGL((pra::xent_bwd_kernel<LT>), dim3(T), dim3(256), 0, s, (LT*)logits, labels,
                                        lse, stats, grad_out, V, ld, ignore_index));
  return hipGetLastError();
}

// stats: float[8] device buffer (xent_reduce_reg_kernel); nll_row / smooth_row: float[T] work buffers
hipError_t pra_xent_fwd_reg(int dtype, const void* logits, const int64_t* labels, float* lse, float* nll_row,
                            float* smooth_row, float* stats, long T, long V, long ld, long ignore_index, double z_loss,
                            double label_smoothing, hipStream_t s) {
  if (ld % 8) return hipErrorInvalidValue;
  if (label_smoothing > 0.0) {
    PRA_DISPATCH_FLOAT(dtype, LT,
                       hipLaunchKernelGGL((pra::xent_fwd_reg_kernel<LT, true>), dim3(T), dim3(256), 0, s,
                                          (const LT*)logits, labels, lse, nll_row, smooth_row, V, ld, ignore_index));
  } else {
    PRA_DISPATCH_FLOAT(dtype, LT,
                       hipLaunchKernelGGL((pra::xent_fwd_reg_kernel<LT, false>), dim3(T), dim3(256), 0, s,
                                          (const LT*)logits, labels, lse, nll_row, smooth_row, V, ld, ignore_index));
  }
  hipLaunchKernelGGL(pra::xent_reduce_reg_kernel, dim3(1), dim3(256), 0, s, nll_row, smooth_row, lse, labels, stats, T,
                     V, ignore_index, (float)z_loss, (float)label_smoothing);
  return hipGetLastError();
}

hipError_t pra_xent_bwd_reg(int dtype, void* logits, const int64_t* labels, const float* lse, const float* stats,
                            const float* grad_out, long T, long V, long ld, long ignore_index, double z_loss,
                            double label_smoothing, hipStream_t s) {
  if (ld % 8) return hipErrorInvalidValue;
  const float off = (float)(label_smoothing / (double)V);
  const float on = (float)((1.0 - label_smoothing) + label_smoothing / (double)V);
  PRA_DISPATCH_FLOAT(dtype, LT,
                     hipLaunchKernelGGL((pra::xent_bwd_reg_kernel<LT>), dim3(T), dim3(256), 0, s, (LT*)logits, labels,
                                        lse, stats, grad_out, V, ld, ignore_index, (float)z_loss, on, off));
  return hipGetLastError();
}

}  // extern "C"
