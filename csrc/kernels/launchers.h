// C ABI of the HIP kernels in csrc/kernels/*.hip. The kernel translation units do not include
// any torch header; csrc/bindings.cpp adapts torch tensors to these raw-pointer launchers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "attn_plan.h"
#include "gemm_plan.h"

extern "C" {
int pra_rmsnorm_bwd_ws_extra();
int pra_rmsnorm_bwd_ws_rows(int rows);
hipError_t pra_rmsnorm_fwd(int dtype, const void* x, const void* delta, const void* w, void* h_out, void* y,
                           float* rstd, int rows, int D, float eps, hipStream_t s);
hipError_t pra_rmsnorm_bwd(int dtype, const void* dy, const void* h, const void* w, const float* rstd,
                           const void* dres, void* dx, void* dw, float* ws, int rows, int D, int accumulate,
                           hipStream_t s);

hipError_t pra_layernorm_fwd(int dtype, const void* x, const void* delta, const void* w, const void* b, void* h_out,
                             void* y, float* mean, float* rstd, int rows, int D, float eps, hipStream_t s);
hipError_t pra_layernorm_bwd(int dtype, const void* dy, const void* h, const void* w, const float* mean,
                             const float* rstd, const void* dres, void* dx, void* dwb, float* ws, int rows, int D,
                             int accumulate, hipStream_t s);

// doc_start (optional, int32 [ntok]): packed sequences, table row (t % S) - doc_start[t]
hipError_t pra_rope(int dtype, void* x, const void* tab, long ntok, int ld, int ncols, int D, int S,
                    int pos_offset, int inverse, const int* doc_start, hipStream_t s);
hipError_t pra_swiglu_fwd(int dtype, const void* g, const void* u, void* y, long ntok, int F, int ldg, int ldu,
                          int ldy, hipStream_t s);
hipError_t pra_swiglu_bwd(int dtype, const void* dy, const void* g, const void* u, void* dg, void* du, long ntok,
                          int F, int ldg, int ldu, int lddy, int variant, hipStream_t s);
hipError_t pra_embedding_fwd(int dtype, const int64_t* ids, const void* W, void* out, long ntok, int D, long V,
                             hipStream_t s);
hipError_t pra_embedding_bwd(int dtype, const int64_t* sorted_ids, const int64_t* perm, const void* dout, void* dW,
                             long ntok, int D, long V, int accumulate, hipStream_t s);

hipError_t pra_swiglu_fwd_t(int dtype, const void* gu, void* a, void* aT, long ntok, int F, int ldgu, int lda,
                            hipStream_t s);
hipError_t pra_swiglu_bwd_t(int dtype, const void* dy, void* gu, void* guT, long ntok, int F, int ldgu, int lddy,
                            hipStream_t s);
hipError_t pra_rope_t(int dtype, void* x, void* xT, const void* tab, long ntok, int ld, int ncols, int nrot, int D,
                      int S, int inverse, hipStream_t s);
hipError_t pra_transpose16(const void* src, void* dst, long R, long C, long ld_src, long ld_dst, hipStream_t s);
// The hand-written GEMMs, bf16 / fp16, M and N multiples of 256, K of 32, leading dimensions in elements
// (% 8). The launchers read the block before they return and keep no pointer to it (graph capture).
//   pra_gemm_nt (gemm_nt.hip):       C[M][N] = A B^T with A [M][K], B [N][K], both K-contiguous, and a
//                                    fused epilogue; accumulate must be 0
//   pra_wgrad_gemm (gemm_wgrad.hip): C[M][N] (+)= A^T B with A [K][M], B [K][N] row-major (the weight
//                                    gradient on row-major activations); epi must be 0
typedef struct pra_gemm_args {
  int dtype;  // pra::kBF16 / kF16
  int M, N, K;
  const void* a; long lda;
  const void* b; long ldb;
  void* c; long ldc;
  int accumulate;  // weight gradient: add the existing C in fp32 and round once (addmm's beta = 1)
  // NT epilogue: 0 plain; 1 SwiGLU forward (b = W1|W3 [2F][K], c = gu [M][2F] with N = 2F, c2 = a [M][F]);
  // 2 SwiGLU backward in place over c = gu [M][2F] (N = F, ldc >= 2F; da itself is never stored);
  // 3 RoPE on the first nrot columns of c
  int epi;
  void* c2; long ldc2;  // epi 1: a = round(silu(g)) * u
  int F;                // epi 1 / 2: gu holds g at [0, F) and u at [F, 2F)
  const void* tab;      // epi 3: (cos, sin) float2 [S][D / 2]
  int S, D, nrot;       // epi 3: row m sits at position m % S; head dim D % 8 == 0; nrot % D == 0, <= N
  // Split tail (gemm_plan.h): pra_gemm_scratch floats / int32s, uninitialised. Either null: the tail
  // tiles run unsplit.
  float* ws;
  int* tickets;
  int cus;  // compute units of the device
} pra_gemm_args;
hipError_t pra_gemm_nt(const pra_gemm_args* a, hipStream_t s);
hipError_t pra_wgrad_gemm(const pra_gemm_args* a, hipStream_t s);
// kind: pra::GemmKind. Fills the fp32 floats and the tickets the split tail of an [M, N, K] GEMM takes
// (both 0: no split)
void pra_gemm_scratch(int kind, int M, int N, int K, int cus, long* ws_floats, int* tickets);

hipError_t pra_xent_fwd(int dtype, const void* logits, const int64_t* labels, float* lse, float* loss_row,
                        float* stats, long T, long V, long ld, long ignore_index, hipStream_t s);
hipError_t pra_xent_bwd(int dtype, void* logits, const int64_t* labels, const float* lse, const float* stats,
                        const float* grad_out, long T, long V, long ld, long ignore_index, hipStream_t s);
// regularised objective (z-loss, label smoothing) and logit telemetry; stats is float[8]
hipError_t pra_xent_fwd_reg(int dtype, const void* logits, const int64_t* labels, float* lse, float* nll_row,
                            float* smooth_row, float* stats, long T, long V, long ld, long ignore_index, double z_loss,
                            double label_smoothing, hipStream_t s);
hipError_t pra_xent_bwd_reg(int dtype, void* logits, const int64_t* labels, const float* lse, const float* stats,
                            const float* grad_out, long T, long V, long ld, long ignore_index, double z_loss,
                            double label_smoothing, hipStream_t s);

// Stochastic rounding of a 16-bit AdamW launch (philox_sr.h). mask 0: round to nearest, the rest is unused.
typedef struct pra_sr_args {
  unsigned long long seed;  // Philox key
  long long base;           // flat position of the launch's first element (>= 0, % 8 == 0)
  int step;                 // AdamW step number (1-based: the one the bias corrections use) ...
  const int* step_dev;      // ... or, when non-null, read from device memory (guard / graph mode)
  int mask;                 // bit 0: round p stochastically, bit 1: exp_avg, bit 2: exp_avg_sq
} pra_sr_args;
// Everything launch-uniform of an AdamW update (optim.hip documents the math and the device scalars).
// The launchers copy the block before they return and keep no pointer to it (graph capture).
typedef struct pra_adamw_args {
  double lr, b1, b2, eps, wd, bc1, bc2_sqrt;
  float gscale;             // gradient multiplier, times gscale_dev[0] when that is non-null
  int fast;                 // hardware reciprocal / square root instead of torch's exact expression tree
  const float* gscale_dev;  // optional device scalars: fp32[1],
  const double* hyper_dev;  //   fp64[3] = {lr, bc1, bc2_sqrt} replacing the host values,
  const int* skip_dev;      //   int32[1], non-zero: the launch does nothing
  pra_sr_args sr;           // non-zero mask: 16-bit state only, not the master launcher
} pra_adamw_args;
// pdtype: param/grad dtype; sdtype: moment dtype (the same: all fp32 or all one 16-bit type)
hipError_t pra_adamw_flat(int pdtype, int sdtype, void* p, const void* g, void* m, void* v, long n,
                          const pra_adamw_args* args, hipStream_t s);
// fp32-master AdamW: updates pm / m / v (fp32) and writes p = round(pm) (16-bit params)
hipError_t pra_adamw_master(int pdtype, void* p, float* pm, const void* g, float* m, float* v, long n,
                            const pra_adamw_args* args, hipStream_t s);
// AdamW of one row-major [rows, cols] matrix that also writes pt = p^T [cols, rows] (rows, cols % 64 == 0,
// 16-bit p / g / m / v / pt of one dtype); with sr.mask, pt takes the rounded p
hipError_t pra_adamw_t(int dtype, void* p, const void* g, void* m, void* v, void* pt, int rows, int cols,
                       const pra_adamw_args* args, hipStream_t s);
int pra_sumsq_partials();
hipError_t pra_grad_norm(int dtype, const void* x, long n, float* ws, float* out, float max_norm, float pre_scale,
                         hipStream_t s);
// loss-scale / non-finite guard: grad_norm's reduction (or sq_dev, fp64[1]) + the skip decision and scale
// state machine on the device (optim.hip guard_finish_kernel documents state / out / hyper)
hipError_t pra_guard_step(int dtype, const void* x, long n, const double* sq_dev, float* ws, int* state, float* out,
                          double* hyper, float max_norm, float pre_scale, int dynamic, int interval, double b1,
                          double b2, hipStream_t s);

// dst <- src, nbytes, device memory (16-B vector path when both are 16-B aligned)
hipError_t pra_copy_d2d(void* dst, const void* src, long nbytes, hipStream_t s);
int pra_checksum_blocks();
hipError_t pra_checksum(int dtype, const void* x, long nbytes, double* ws_sum, unsigned long long* ws_hash,
                        double* out_sum, unsigned long long* out_hash, hipStream_t s);
hipError_t pra_sum_slices(int dtype, const void* const* srcs, int nsrc, void* dst, long n, hipStream_t s);
// n (<= 16) copies src[k] -> dst[k] of nbytes[k] in one kernel (16-B aligned pointers)
hipError_t pra_pull_gather(const void* const* srcs, void* const* dsts, const long* nbytes, int n, hipStream_t s);
// sparse embedding-gradient exchange over W (<= 16) dense [V, D] gradients and W sorted id lists of n
// int64 entries: phase 1 reduces the union rows rank `me` owns into grads[me], phase 2 copies the others
hipError_t pra_sparse_rows(int dtype, int phase, void* const* grads, const int64_t* const* ids, int W, int me, long n,
                           long V, long D, hipStream_t s);

// Training attention (attention.hip and its siblings). Tensors are [B, S, H, D] views with a token
// stride in elements (% 8 for bf16 / fp16, % 4 for fp32), so q / k / v can be slices of a fused QKV
// activation; lse is fp32 [B, Hq, S]. The launchers read the block before they return and keep no
// pointer to it (graph capture).
typedef struct pra_attn_args {
  int dtype;  // pra::DType: kF32 routes to the fp32 kernels (attention_f32.hip)
  int B, S, Hq, Hkv, D;
  int skv;     // real sequence length when S is zero-padded (keys >= skv are masked), else S
  int causal;
  float scale;
  const void* q; long ldq;
  const void* k; long ldk;
  const void* v; long ldv;
  void* o; long ldo;  // written by the forward, read by the backward
  const void* dout; long lddo;
  void* dq; long lddq;
  void* dk; long lddk;
  void* dv; long lddv;
  float* lse;  // written by the forward, read by the backward
  float* ws;   // backward: pra_attn_bwd_workspace floats
  // The rest is optional. doc_start, int32 [B][S]: document-masked causal attention (attention_docs.hip,
  // 16-bit, S % 128 == 0): query i sees key j iff doc_start[b][i] <= j <= i (values clamped into [0, i]).
  // rope_tab (16-bit), fp32 [>= S][D / 2][2]: dq / dk are stored with the inverse rotation (with doc_start:
  // at the packed positions i - doc_start[b][i]). mid_event: recorded once where a side-stream job may
  // start beside the backward (BwdPlan::win_early; docs: between dQ and dK/dV; fp32: never).
  const int* doc_start;
  const float* rope_tab;
  hipEvent_t mid_event;
} pra_attn_args;
hipError_t pra_attn_fwd(const pra_attn_args* a, hipStream_t st);
hipError_t pra_attn_bwd(const pra_attn_args* a, hipStream_t st);
// floats of fp32 workspace pra_attn_bwd needs at `ws` (shape, dtype and doc_start != null are read)
long pra_attn_bwd_workspace(const pra_attn_args* a);
// kernel selection (attn_plan.h); not thread-safe against concurrent launches (set between steps)
void pra_attn_get_options(pra_attn_options* out);
void pra_attn_set_options(const pra_attn_options* in);

// KV-cache generation (attention_decode.hip), bf16 / fp16. Caches are [B][cap][Hkv][D] contiguous;
// kv_len is int32 [B] on the device and is clamped by the kernels (no host copy is ever read).
// rope_append: qkv [B * nt][ld] = q | k | v of nt new tokens per sequence, row b * nt + t at position
// p = clamp(kv_len[b], 0, cap) + t; rotates q in place, writes rotated k and plain v into cache row p.
// nt == 1: the row is clamp(kv_len[b], 0, cap - 1). nt > 1: a row with p >= cap stores nothing and its q
// is rotated with table row cap - 1. tab: float2 [>= cap][D/2].
hipError_t pra_rope_append(int dtype, void* qkv, const void* tab, const int* kv_len, void* k_cache, void* v_cache,
                           int B, int nt, long ld, int Hq, int Hkv, int D, int cap, hipStream_t s);
// q, o [B][Hq][D] contiguous, lse fp32 [B][Hq]; sequence b attends to keys 0 .. clamp(kv_len[b], 0, cap) - 1.
// D 64 or 128. ws: pra_attn_decode_ws_floats fp32 words. pra_attn_decode_chunk: keys per chunk.
hipError_t pra_attn_decode(int dtype, const void* q, const void* k_cache, const void* v_cache, const int* kv_len,
                           void* o, float* lse, float* ws, int B, int Hq, int Hkv, int D, int cap, float scale,
                           hipStream_t s);
long pra_attn_decode_ws_floats(int B, int Hq, int D, int cap);
int pra_attn_decode_chunk();
// the merge of pra_attn_decode alone: ws_o [B][Hq][NC][D], ws_ml [B][Hq][NC][2], NC = ceil(cap / chunk)
hipError_t pra_attn_decode_combine(int dtype, const float* ws_o, const float* ws_ml, const int* kv_len, void* o,
                                   float* lse, int B, int Hq, int D, int cap, int NC, hipStream_t s);

// Multi-token append (attention_extend.hip), bf16 / fp16, D 64 or 128. q: T queries per sequence, row
// b * T + t of a [B * T][ldq] view (Hq * D columns, ldq % 8 == 0); query t of sequence b attends to keys
// 0 .. min(clamp(kv_len[b], 0, cap) + t, cap - 1) of the caches, which hold the new tokens' k / v already
// (pra_rope_append with nt = T runs first). o [B][T][Hq][D] contiguous, lse fp32 [B][T][Hq].
hipError_t pra_attn_extend(int dtype, const void* q, long ldq, const void* k_cache, const void* v_cache,
                           const int* kv_len, void* o, float* lse, int B, int T, int Hq, int Hkv, int D, int cap,
                           float scale, hipStream_t s);

// fp8 KV cache (attention_decode_fp8.hip documents the format): k_cache, v_cache uint8 [B][cap][Hkv][D] of
// e4m3fn bytes, k_scale, v_scale fp32 [B][cap][Hkv], powers of two. dtype is the 16-bit type of qkv / q / o.
// D 64 or 128. kv_quantize: k, v [B * S][ld] views of the fused QKV activation (Hkv * D columns each,
// ld % 8 == 0) into cache rows 0 .. S - 1 (S <= cap). rope_append_fp8 and attn_decode_fp8 are
// pra_rope_append / pra_attn_decode over this cache, same workspace.
hipError_t pra_kv_quantize(int dtype, const void* k, const void* v, long ld, void* k_cache, void* v_cache,
                           float* k_scale, float* v_scale, int B, int S, int Hkv, int D, int cap, hipStream_t s);
hipError_t pra_rope_append_fp8(int dtype, void* qkv, const void* tab, const int* kv_len, void* k_cache, void* v_cache,
                               float* k_scale, float* v_scale, int B, long ld, int Hq, int Hkv, int D, int cap,
                               hipStream_t s);
hipError_t pra_attn_decode_fp8(int dtype, const void* q, const void* k_cache, const void* v_cache,
                               const float* k_scale, const float* v_scale, const int* kv_len, void* o, float* lse,
                               float* ws, int B, int Hq, int Hkv, int D, int cap, float scale, hipStream_t s);
int pra_attn_decode_fp8_chunk();

// Device-side sampling (sample.hip documents the rule), bf16 / fp16 logits [B][ld], ld >= V >= 1, no
// alignment demand beyond the element. The launcher copies the block before it returns (graph capture).
// The generation state is optional (done == null: absent). With it the launch also does the bookkeeping
// of inference.generate: a row with done[b] set writes nothing but tok[b] = 0; any other row stores its
// token at out[b][count[b]], increments count[b], and sets done[b] when the token is eos_id or
// count[b] > room[b] (room: cache rows the sequence had left after its prompt; the token that finds the
// cache full is still emitted). tok[b] of a row that finished in this launch is 0 too: tok is the next
// decode step's input.
typedef struct pra_sample_state {
  unsigned char* done;    // uint8 [B]
  int* count;             // int32 [B]: tokens emitted so far
  const int* room;        // int32 [B]
  long long* out;         // int64 [B][max_new]
  int max_new;
  long long eos_id;       // -1: none
  const int* prompt_len;  // optional int32 [B]: the draw's position is prompt_len[b] + count[b], not pos[b]
} pra_sample_state;
typedef struct pra_sample_args {
  float temperature;  // 0: greedy under NaN < -inf < finite < +inf, ties to the lowest id; no Philox call
  int top_k;          // 0: off
  float top_p;        // in (0, 1]
  unsigned long long seed;
  const int* pos;     // int32 [B]: absolute position the sampled token will occupy (Philox counter word 1)
  long long* tok;     // int64 [B], output
  float* u_out;       // optional fp32 [B]: the uniform each row drew (temperature > 0)
  unsigned* ws;       // pra_sample_ws_bytes(B) bytes, 16-B aligned, any contents (temperature > 0)
  pra_sample_state gen;
} pra_sample_args;
long pra_sample_ws_bytes(int B);
hipError_t pra_sample(int dtype, const void* logits, long ld, int B, int V, const pra_sample_args* args,
                      hipStream_t s);
}
