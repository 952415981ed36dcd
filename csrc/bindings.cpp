// Torch <-> HIP kernel adapter for pyrecover_amd._C.
//
// Every op validates shapes/strides/dtypes on the host BEFORE launching (a mis-shaped launch
// of a hand-written kernel could fault the GPU), then calls the raw launcher on the current
// HIP stream of the tensor's device.
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <c10/core/DeviceGuard.h>

#include <roctracer/roctx.h>

#include <atomic>
#include <cstdlib>

#include "kernels/launchers.h"

namespace {

// roctx range per op ("pyrecover::attn_fwd", ...) so rocprofv3 --marker-trace / --selected-regions
// timelines show which framework op launched each kernel. Off by default (one branch per op);
// enabled by set_roctx(True) (train.py --profile) or PYRECOVER_ROCTX=1.
std::atomic<bool> g_roctx{[] {
  const char* e = std::getenv("PYRECOVER_ROCTX");
  return e != nullptr && e[0] == '1';
}()};
struct Range {
  bool on;
  explicit Range(const char* name) : on(g_roctx.load(std::memory_order_relaxed)) {
    if (on) roctxRangePushA(name);
  }
  ~Range() {
    if (on) roctxRangePop();
  }
};

int dt(const at::Tensor& t) {
  switch (t.scalar_type()) {
    case at::kFloat: return 0;
    case at::kBFloat16: return 1;
    case at::kHalf: return 2;
    default: TORCH_CHECK(false, "pyrecover_amd: unsupported dtype ", t.scalar_type());
  }
}

hipStream_t stream_of(const at::Tensor& t) {
  return c10::hip::getCurrentHIPStream(t.device().index()).stream();
}

void check(hipError_t e, const char* what) {
  TORCH_CHECK(e == hipSuccess, "pyrecover_amd: ", what, " failed: ", hipGetErrorString(e));
}

void check_dev(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), "pyrecover_amd: ", name, " must be a GPU tensor");
}

// Every pointer handed to a kernel must live on the launch device (a host or foreign-device
// pointer in a kernel argument is a GPU memory fault, not an exception).
void same_dev(const at::Tensor& ref, const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.defined() && t.is_cuda() && t.device() == ref.device(), "pyrecover_amd: ", name,
              " must be on ", ref.device(), " (got ", t.defined() ? t.device().str() : std::string("undefined"), ")");
}

void check_row_major(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.dim() == 2 && t.stride(1) == 1, "pyrecover_amd: ", name, " must be 2-D with unit inner stride");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, "pyrecover_amd: ", name, " must be 16-B aligned");
}

// ---------------------------------------------------------------------------------------
std::vector<at::Tensor> rmsnorm_fwd(const at::Tensor& x, const c10::optional<at::Tensor>& delta, const at::Tensor& w,
                                    double eps) {
  const Range range_("pyrecover::rmsnorm_fwd");
  check_dev(x, "x");
  TORCH_CHECK(x.is_contiguous() && w.is_contiguous(), "rmsnorm_fwd: x and w must be contiguous");
  const int64_t D = x.size(-1);
  const int64_t rows = x.numel() / D;
  TORCH_CHECK(w.numel() == D && w.scalar_type() == x.scalar_type(), "rmsnorm_fwd: weight mismatch");
  same_dev(x, w, "rmsnorm weight");
  if (delta.has_value()) same_dev(x, *delta, "rmsnorm delta");
  TORCH_CHECK(D % 8 == 0 && D <= 8192, "rmsnorm_fwd: D must be a multiple of 8 and <= 8192");
  const c10::DeviceGuard guard(x.device());
  at::Tensor y = at::empty_like(x);
  at::Tensor rstd = at::empty({rows}, x.options().dtype(at::kFloat));
  at::Tensor h;
  const void* dptr = nullptr;
  if (delta.has_value()) {
    TORCH_CHECK(delta->sizes() == x.sizes() && delta->is_contiguous() && delta->scalar_type() == x.scalar_type(),
                "rmsnorm_fwd: delta mismatch");
    h = at::empty_like(x);
    dptr = delta->data_ptr();
  }
  check(pra_rmsnorm_fwd(dt(x), x.data_ptr(), dptr, w.data_ptr(), h.defined() ? h.data_ptr() : nullptr,
                        y.data_ptr(), rstd.data_ptr<float>(), (int)rows, (int)D, (float)eps, stream_of(x)),
        "rmsnorm_fwd");
  return {h.defined() ? h : x, y, rstd};
}

at::Tensor rmsnorm_bwd(const at::Tensor& dy, const at::Tensor& h, const at::Tensor& w, const at::Tensor& rstd,
                       const c10::optional<at::Tensor>& dres, at::Tensor dw, bool accumulate) {
  const Range range_("pyrecover::rmsnorm_bwd");
  check_dev(dy, "dy");
  TORCH_CHECK(dy.is_contiguous() && h.is_contiguous() && dy.sizes() == h.sizes(), "rmsnorm_bwd: dy/h mismatch");
  const int64_t D = h.size(-1);
  const int64_t rows = h.numel() / D;
  TORCH_CHECK(w.numel() == D && dw.numel() == D && dw.is_contiguous() && rstd.numel() == rows,
              "rmsnorm_bwd: shape mismatch");
  TORCH_CHECK(dw.scalar_type() == h.scalar_type() && dy.scalar_type() == h.scalar_type(), "rmsnorm_bwd: dtype");
  TORCH_CHECK(rstd.scalar_type() == at::kFloat && rstd.is_contiguous(), "rmsnorm_bwd: rstd must be contiguous fp32");
  TORCH_CHECK(D % 8 == 0 && D <= 8192, "rmsnorm_bwd: D must be a multiple of 8 and <= 8192");
  same_dev(dy, h, "h");
  same_dev(dy, w, "w");
  same_dev(dy, rstd, "rstd");
  same_dev(dy, dw, "dw");
  if (dres.has_value()) same_dev(dy, *dres, "dres");
  const c10::DeviceGuard guard(h.device());
  at::Tensor dx = at::empty_like(h);
  const void* dr = nullptr;
  if (dres.has_value()) {
    TORCH_CHECK(dres->sizes() == h.sizes() && dres->is_contiguous() && dres->scalar_type() == h.scalar_type(),
                "rmsnorm_bwd: dres mismatch");
    dr = dres->data_ptr();
  }
  const int wsr = pra_rmsnorm_bwd_ws_rows((int)rows);
  at::Tensor ws = at::empty({wsr + pra_rmsnorm_bwd_ws_extra(), D}, h.options().dtype(at::kFloat));
  check(pra_rmsnorm_bwd(dt(h), dy.data_ptr(), h.data_ptr(), w.data_ptr(), rstd.data_ptr<float>(), dr, dx.data_ptr(),
                        dw.data_ptr(), ws.data_ptr<float>(), (int)rows, (int)D, accumulate ? 1 : 0, stream_of(h)),
        "rmsnorm_bwd");
  return dx;
}

// LayerNorm: returns (h, y, mean, rstd)
std::vector<at::Tensor> layernorm_fwd(const at::Tensor& x, const c10::optional<at::Tensor>& delta, const at::Tensor& w,
                                      const at::Tensor& b, double eps) {
  const Range range_("pyrecover::layernorm_fwd");
  check_dev(x, "x");
  TORCH_CHECK(x.is_contiguous() && w.is_contiguous() && b.is_contiguous(), "layernorm_fwd: contiguous");
  const int64_t D = x.size(-1);
  const int64_t rows = x.numel() / D;
  TORCH_CHECK(w.numel() == D && b.numel() == D && w.scalar_type() == x.scalar_type() &&
              b.scalar_type() == x.scalar_type(), "layernorm_fwd: weight/bias mismatch");
  TORCH_CHECK(D % 8 == 0 && D <= 8192, "layernorm_fwd: D must be a multiple of 8 and <= 8192");
  same_dev(x, w, "weight");
  same_dev(x, b, "bias");
  if (delta.has_value()) {
    TORCH_CHECK(delta->sizes() == x.sizes() && delta->is_contiguous() && delta->scalar_type() == x.scalar_type(),
                "layernorm_fwd: delta mismatch");
    same_dev(x, *delta, "delta");
  }
  const c10::DeviceGuard guard(x.device());
  at::Tensor y = at::empty_like(x);
  auto fo = x.options().dtype(at::kFloat);
  at::Tensor mean = at::empty({rows}, fo), rstd = at::empty({rows}, fo);
  at::Tensor h = delta.has_value() ? at::empty_like(x) : x;
  check(pra_layernorm_fwd(dt(x), x.data_ptr(), delta.has_value() ? delta->data_ptr() : nullptr, w.data_ptr(),
                          b.data_ptr(), delta.has_value() ? h.data_ptr() : nullptr, y.data_ptr(), mean.data_ptr<float>(),
                          rstd.data_ptr<float>(), (int)rows, (int)D, (float)eps, stream_of(x)),
        "layernorm_fwd");
  return {h, y, mean, rstd};
}

// dwb: 2*D contiguous output [dw | db]
at::Tensor layernorm_bwd(const at::Tensor& dy, const at::Tensor& h, const at::Tensor& w, const at::Tensor& mean,
                         const at::Tensor& rstd, const c10::optional<at::Tensor>& dres, at::Tensor dwb, bool accumulate) {
  const Range range_("pyrecover::layernorm_bwd");
  check_dev(dy, "dy");
  TORCH_CHECK(dy.is_contiguous() && h.is_contiguous() && dy.sizes() == h.sizes(), "layernorm_bwd: dy/h mismatch");
  const int64_t D = h.size(-1);
  const int64_t rows = h.numel() / D;
  TORCH_CHECK(w.numel() == D && dwb.numel() == 2 * D && dwb.is_contiguous() && rstd.numel() == rows &&
              mean.numel() == rows, "layernorm_bwd: shapes");
  TORCH_CHECK(dwb.scalar_type() == h.scalar_type() && dy.scalar_type() == h.scalar_type() &&
              rstd.scalar_type() == at::kFloat && mean.scalar_type() == at::kFloat, "layernorm_bwd: dtypes");
  TORCH_CHECK(D % 8 == 0 && D <= 8192, "layernorm_bwd: D must be a multiple of 8 and <= 8192");
  for (const at::Tensor& t : {h, w, mean, rstd, dwb}) same_dev(dy, t, "layernorm operand");
  if (dres.has_value()) {
    TORCH_CHECK(dres->sizes() == h.sizes() && dres->is_contiguous() && dres->scalar_type() == h.scalar_type(),
                "layernorm_bwd: dres");
    same_dev(dy, *dres, "dres");
  }
  const c10::DeviceGuard guard(h.device());
  at::Tensor dx = at::empty_like(h);
  const int wsr = pra_rmsnorm_bwd_ws_rows((int)rows);
  at::Tensor ws = at::empty({wsr + pra_rmsnorm_bwd_ws_extra(), 2 * D}, h.options().dtype(at::kFloat));
  check(pra_layernorm_bwd(dt(h), dy.data_ptr(), h.data_ptr(), w.data_ptr(), mean.data_ptr<float>(),
                          rstd.data_ptr<float>(), dres.has_value() ? dres->data_ptr() : nullptr, dx.data_ptr(),
                          dwb.data_ptr(), ws.data_ptr<float>(), (int)rows, (int)D, accumulate ? 1 : 0, stream_of(h)),
        "layernorm_bwd");
  return dx;
}

// In-place RoPE on the first `ncols` columns of each row of a 2-D [tokens, ld] buffer.
// doc_start (optional, int32 [B, S] with B * S = tokens): packed sequences, positions restart per document.
void rope_(at::Tensor x2d, int64_t ncols, const at::Tensor& tab, int64_t head_dim, int64_t seq_len,
           int64_t pos_offset, bool inverse, const c10::optional<at::Tensor>& doc_start) {
  const Range range_("pyrecover::rope");
  check_dev(x2d, "x");
  check_row_major(x2d, "rope x");
  TORCH_CHECK(tab.scalar_type() == at::kFloat && tab.is_contiguous(), "rope: table must be contiguous fp32");
  same_dev(x2d, tab, "rope table");
  TORCH_CHECK(tab.numel() >= (seq_len + pos_offset) * head_dim, "rope: table too small");
  TORCH_CHECK(ncols <= x2d.size(1) && ncols % head_dim == 0 && head_dim % 8 == 0, "rope: bad ncols/head_dim");
  TORCH_CHECK(x2d.size(0) % seq_len == 0, "rope: tokens must be a multiple of seq_len");
  const int* ds = nullptr;
  if (doc_start.has_value()) {
    TORCH_CHECK(doc_start->scalar_type() == at::kInt && doc_start->is_contiguous() &&
                    doc_start->numel() == x2d.size(0) && doc_start->size(-1) == seq_len,
                "rope: doc_start must be contiguous int32 [tokens / seq_len, seq_len]");
    same_dev(x2d, *doc_start, "doc_start");
    ds = doc_start->data_ptr<int>();
  }
  const c10::DeviceGuard guard(x2d.device());
  check(pra_rope(dt(x2d), x2d.data_ptr(), tab.data_ptr(), x2d.size(0), (int)x2d.stride(0), (int)ncols, (int)head_dim,
                 (int)seq_len, (int)pos_offset, inverse ? 1 : 0, ds, stream_of(x2d)),
        "rope");
}

// gu: [T, 2F] (gate | up) -> y [T, F]
at::Tensor swiglu_fwd(const at::Tensor& gu) {
  const Range range_("pyrecover::swiglu_fwd");
  check_dev(gu, "gu");
  check_row_major(gu, "gu");
  TORCH_CHECK(gu.size(1) % 16 == 0, "swiglu: 2F must be a multiple of 16");
  const int64_t F = gu.size(1) / 2;
  const c10::DeviceGuard guard(gu.device());
  at::Tensor y = at::empty({gu.size(0), F}, gu.options());
  const char* base = (const char*)gu.data_ptr();
  check(pra_swiglu_fwd(dt(gu), base, base + F * gu.element_size(), y.data_ptr(), gu.size(0), (int)F,
                       (int)gu.stride(0), (int)gu.stride(0), (int)F, stream_of(gu)),
        "swiglu_fwd");
  return y;
}

// dgu may alias gu (in-place backward).
at::Tensor swiglu_bwd(const at::Tensor& dy, const at::Tensor& gu, c10::optional<at::Tensor> out, int64_t variant) {
  const Range range_("pyrecover::swiglu_bwd");
  check_dev(gu, "gu");
  check_row_major(gu, "gu");
  check_row_major(dy, "dy");
  const int64_t F = gu.size(1) / 2;
  TORCH_CHECK(dy.size(0) == gu.size(0) && dy.size(1) == F && dy.scalar_type() == gu.scalar_type(), "swiglu_bwd: dy");
  same_dev(gu, dy, "dy");
  if (out.has_value()) same_dev(gu, *out, "out");
  const c10::DeviceGuard guard(gu.device());
  at::Tensor dgu = out.has_value() ? *out : at::empty_like(gu);
  TORCH_CHECK(dgu.sizes() == gu.sizes() && dgu.strides() == gu.strides(), "swiglu_bwd: out layout");
  const char* g = (const char*)gu.data_ptr();
  char* o = (char*)dgu.data_ptr();
  const int64_t es = gu.element_size();
  check(pra_swiglu_bwd(dt(gu), dy.data_ptr(), g, g + F * es, o, o + F * es, gu.size(0), (int)F, (int)gu.stride(0),
                       (int)gu.stride(0), (int)dy.stride(0), (int)variant, stream_of(gu)),
        "swiglu_bwd");
  return dgu;
}

// gu: [T, 2F] -> (a [T, F], a^T [F, T]) in one pass (same math as swiglu_fwd).
std::vector<at::Tensor> swiglu_fwd_t(const at::Tensor& gu) {
  const Range range_("pyrecover::swiglu_fwd_t");
  check_dev(gu, "gu");
  check_row_major(gu, "gu");
  const int64_t T = gu.size(0), F = gu.size(1) / 2;
  TORCH_CHECK(gu.element_size() == 2, "swiglu_fwd_t: 16-bit dtype required");
  TORCH_CHECK(T % 64 == 0 && F % 64 == 0 && gu.size(1) == 2 * F, "swiglu_fwd_t: tokens and F must be multiples of 64");
  const c10::DeviceGuard guard(gu.device());
  at::Tensor a = at::empty({T, F}, gu.options());
  at::Tensor aT = at::empty({F, T}, gu.options());
  check(pra_swiglu_fwd_t(dt(gu), gu.data_ptr(), a.data_ptr(), aT.data_ptr(), T, (int)F, (int)gu.stride(0), (int)F,
                         stream_of(gu)),
        "swiglu_fwd_t");
  return {a, aT};
}

// In place: gu <- [dg | du] (the SwiGLU backward, same math as swiglu_bwd); returns dgu^T [2F, T].
at::Tensor swiglu_bwd_t_(const at::Tensor& dy, at::Tensor gu) {
  const Range range_("pyrecover::swiglu_bwd_t");
  check_dev(gu, "gu");
  check_row_major(gu, "gu");
  check_row_major(dy, "dy");
  const int64_t T = gu.size(0), F = gu.size(1) / 2;
  TORCH_CHECK(gu.element_size() == 2, "swiglu_bwd_t: 16-bit dtype required");
  TORCH_CHECK(dy.size(0) == T && dy.size(1) == F && dy.scalar_type() == gu.scalar_type(), "swiglu_bwd_t: dy");
  TORCH_CHECK(T % 64 == 0 && F % 64 == 0, "swiglu_bwd_t: tokens and F must be multiples of 64");
  same_dev(gu, dy, "dy");
  const c10::DeviceGuard guard(gu.device());
  at::Tensor guT = at::empty({2 * F, T}, gu.options());
  check(pra_swiglu_bwd_t(dt(gu), dy.data_ptr(), gu.data_ptr(), guT.data_ptr(), T, (int)F, (int)gu.stride(0),
                         (int)dy.stride(0), stream_of(gu)),
        "swiglu_bwd_t");
  return guT;
}

// In place RoPE (inverse if requested) on the first `nrot` columns of x2d [T, C]; returns x2d^T.
at::Tensor rope_t_(at::Tensor x2d, int64_t nrot, const at::Tensor& tab, int64_t head_dim, int64_t seq_len,
                   bool inverse) {
  const Range range_("pyrecover::rope_t");
  check_dev(x2d, "x");
  check_row_major(x2d, "rope_t x");
  TORCH_CHECK(x2d.element_size() == 2, "rope_t: 16-bit dtype required");
  TORCH_CHECK(tab.scalar_type() == at::kFloat && tab.is_contiguous(), "rope_t: table must be contiguous fp32");
  same_dev(x2d, tab, "rope table");
  TORCH_CHECK(tab.numel() >= seq_len * head_dim, "rope_t: table too small");
  const int64_t T = x2d.size(0), C = x2d.size(1);
  TORCH_CHECK(nrot <= C && nrot % head_dim == 0 && head_dim % 8 == 0, "rope_t: bad nrot/head_dim");
  TORCH_CHECK(T % seq_len == 0 && T % 64 == 0 && C % 64 == 0, "rope_t: shape must tile by 64");
  const c10::DeviceGuard guard(x2d.device());
  at::Tensor xT = at::empty({C, T}, x2d.options());
  check(pra_rope_t(dt(x2d), x2d.data_ptr(), xT.data_ptr(), tab.data_ptr(), T, (int)x2d.stride(0), (int)C, (int)nrot,
                   (int)head_dim, (int)seq_len, inverse ? 1 : 0, stream_of(x2d)),
        "rope_t");
  return xT;
}

at::Tensor embedding_fwd(const at::Tensor& ids, const at::Tensor& W) {
  const Range range_("pyrecover::embedding_fwd");
  check_dev(W, "W");
  TORCH_CHECK(ids.scalar_type() == at::kLong && ids.is_contiguous() && ids.device() == W.device(),
              "embedding: ids must be contiguous int64 on the weight's device");
  TORCH_CHECK(W.dim() == 2 && W.is_contiguous() && W.size(1) % 8 == 0, "embedding: bad weight");
  const c10::DeviceGuard guard(W.device());
  auto sizes = ids.sizes().vec();
  sizes.push_back(W.size(1));
  at::Tensor out = at::empty(sizes, W.options());
  check(pra_embedding_fwd(dt(W), ids.data_ptr<int64_t>(), W.data_ptr(), out.data_ptr(), ids.numel(), (int)W.size(1),
                          W.size(0), stream_of(W)),
        "embedding_fwd");
  return out;
}

// Deterministic dense embedding gradient into dW (overwrites unless accumulate).
void embedding_bwd(const at::Tensor& ids, const at::Tensor& dout, at::Tensor dW, bool accumulate) {
  const Range range_("pyrecover::embedding_bwd");
  check_dev(dW, "dW");
  TORCH_CHECK(dW.is_contiguous() && dout.is_contiguous() && dout.size(-1) == dW.size(1), "embedding_bwd: shapes");
  TORCH_CHECK(dout.numel() / dW.size(1) == ids.numel(), "embedding_bwd: ids/dout mismatch");
  TORCH_CHECK(ids.scalar_type() == at::kLong && dout.scalar_type() == dW.scalar_type(), "embedding_bwd: dtypes");
  same_dev(dW, ids, "ids");
  same_dev(dW, dout, "dout");
  const c10::DeviceGuard guard(dW.device());
  auto flat = ids.reshape({-1});
  auto sorted = at::sort(flat, /*stable=*/true, /*dim=*/0, /*descending=*/false);
  at::Tensor sids = std::get<0>(sorted).contiguous();
  at::Tensor perm = std::get<1>(sorted).contiguous();
  if (!accumulate) dW.zero_();
  check(pra_embedding_bwd(dt(dW), sids.data_ptr<int64_t>(), perm.data_ptr<int64_t>(), dout.data_ptr(), dW.data_ptr(),
                          flat.numel(), (int)dW.size(1), dW.size(0), accumulate ? 1 : 0, stream_of(dW)),
        "embedding_bwd");
}

// The kernels read rows in 8-element vectors from the row start: a V that is not a multiple of 8 must
// be a [:, :V] view of a buffer whose rows are padded to one.
void check_xent_stride(const at::Tensor& logits) {
  TORCH_CHECK(logits.stride(0) % 8 == 0, "xent: the logits row stride must be a multiple of 8 elements (row stride % 8 "
              "== 0), got ", logits.stride(0), " for V = ", logits.size(1), "; pass a [:, :V] view of a padded buffer");
}

// logits [T, V] (row stride ld), labels [T] -> (lse [T], loss_row [T], stats [2] = {mean loss, n_valid})
std::vector<at::Tensor> xent_fwd(const at::Tensor& logits, const at::Tensor& labels, int64_t ignore_index) {
  const Range range_("pyrecover::xent_fwd");
  check_dev(logits, "logits");
  check_row_major(logits, "logits");
  check_xent_stride(logits);
  TORCH_CHECK(labels.scalar_type() == at::kLong && labels.is_contiguous() && labels.numel() == logits.size(0),
              "xent: labels must be contiguous int64 [T]");
  same_dev(logits, labels, "labels");
  const c10::DeviceGuard guard(logits.device());
  const int64_t T = logits.size(0);
  auto fo = logits.options().dtype(at::kFloat);
  at::Tensor lse = at::empty({T}, fo), loss_row = at::empty({T}, fo), stats = at::empty({2}, fo);
  check(pra_xent_fwd(dt(logits), logits.data_ptr(), labels.data_ptr<int64_t>(), lse.data_ptr<float>(),
                     loss_row.data_ptr<float>(), stats.data_ptr<float>(), T, logits.size(1), logits.stride(0),
                     ignore_index, stream_of(logits)),
        "xent_fwd");
  return {lse, loss_row, stats};
}

void xent_bwd_(at::Tensor logits, const at::Tensor& labels, const at::Tensor& lse, const at::Tensor& stats,
               const at::Tensor& grad_out, int64_t ignore_index) {
  const Range range_("pyrecover::xent_bwd");
  check_dev(logits, "logits");
  check_row_major(logits, "logits");
  check_xent_stride(logits);
  TORCH_CHECK(grad_out.scalar_type() == at::kFloat && grad_out.numel() == 1 && grad_out.is_cuda(),
              "xent_bwd: grad_out must be a 1-element fp32 GPU tensor");
  TORCH_CHECK(labels.scalar_type() == at::kLong && labels.is_contiguous() && labels.numel() == logits.size(0),
              "xent_bwd: labels");
  TORCH_CHECK(lse.scalar_type() == at::kFloat && lse.numel() == logits.size(0) && stats.numel() == 2 &&
              stats.scalar_type() == at::kFloat, "xent_bwd: lse/stats");
  same_dev(logits, labels, "labels");
  same_dev(logits, lse, "lse");
  same_dev(logits, stats, "stats");
  same_dev(logits, grad_out, "grad_out");
  const c10::DeviceGuard guard(logits.device());
  check(pra_xent_bwd(dt(logits), logits.data_ptr(), labels.data_ptr<int64_t>(), lse.data_ptr<float>(),
                     stats.data_ptr<float>(), grad_out.data_ptr<float>(), logits.size(0), logits.size(1),
                     logits.stride(0), ignore_index, stream_of(logits)),
        "xent_bwd");
}

void check_xent_coefficients(double z_loss, double label_smoothing) {
  TORCH_CHECK(std::isfinite(z_loss) && z_loss >= 0.0, "xent: z_loss must be finite and >= 0, got ", z_loss);
  TORCH_CHECK(label_smoothing >= 0.0 && label_smoothing < 1.0, "xent: label_smoothing must be in [0, 1), got ",
              label_smoothing);
}

// The regularised objective ((1 - eps) nll + eps smooth + z lse^2, mean over the valid rows) and the logit
// statistics: logits [T, V] (row stride ld), labels [T] -> (lse [T], stats [8] = {objective, n_valid, mean nll,
// z-loss term, mean smooth, mean lse, max |lse|, 0})
std::vector<at::Tensor> xent_fwd_reg(const at::Tensor& logits, const at::Tensor& labels, int64_t ignore_index,
                                     double z_loss, double label_smoothing) {
  const Range range_("pyrecover::xent_fwd_reg");
  check_dev(logits, "logits");
  check_row_major(logits, "logits");
  check_xent_stride(logits);
  check_xent_coefficients(z_loss, label_smoothing);
  TORCH_CHECK(labels.scalar_type() == at::kLong && labels.is_contiguous() && labels.numel() == logits.size(0),
              "xent: labels must be contiguous int64 [T]");
  same_dev(logits, labels, "labels");
  const c10::DeviceGuard guard(logits.device());
  const int64_t T = logits.size(0);
  auto fo = logits.options().dtype(at::kFloat);
  at::Tensor lse = at::empty({T}, fo), rows = at::empty({2, T}, fo), stats = at::empty({8}, fo);
  check(pra_xent_fwd_reg(dt(logits), logits.data_ptr(), labels.data_ptr<int64_t>(), lse.data_ptr<float>(),
                         rows.data_ptr<float>(), rows.data_ptr<float>() + T, stats.data_ptr<float>(), T,
                         logits.size(1), logits.stride(0), ignore_index, z_loss, label_smoothing, stream_of(logits)),
        "xent_fwd_reg");
  return {lse, stats};
}

void xent_bwd_reg_(at::Tensor logits, const at::Tensor& labels, const at::Tensor& lse, const at::Tensor& stats,
                   const at::Tensor& grad_out, int64_t ignore_index, double z_loss, double label_smoothing) {
  const Range range_("pyrecover::xent_bwd_reg");
  check_dev(logits, "logits");
  check_row_major(logits, "logits");
  check_xent_stride(logits);
  check_xent_coefficients(z_loss, label_smoothing);
  TORCH_CHECK(grad_out.scalar_type() == at::kFloat && grad_out.numel() == 1 && grad_out.is_cuda(),
              "xent_bwd: grad_out must be a 1-element fp32 GPU tensor");
  TORCH_CHECK(labels.scalar_type() == at::kLong && labels.is_contiguous() && labels.numel() == logits.size(0),
              "xent_bwd: labels");
  TORCH_CHECK(lse.scalar_type() == at::kFloat && lse.numel() == logits.size(0) && lse.is_contiguous() &&
              stats.numel() == 8 && stats.scalar_type() == at::kFloat && stats.is_contiguous(),
              "xent_bwd_reg: lse must be fp32 [T] and stats fp32 [8]");
  same_dev(logits, labels, "labels");
  same_dev(logits, lse, "lse");
  same_dev(logits, stats, "stats");
  same_dev(logits, grad_out, "grad_out");
  const c10::DeviceGuard guard(logits.device());
  check(pra_xent_bwd_reg(dt(logits), logits.data_ptr(), labels.data_ptr<int64_t>(), lse.data_ptr<float>(),
                         stats.data_ptr<float>(), grad_out.data_ptr<float>(), logits.size(0), logits.size(1),
                         logits.stride(0), ignore_index, z_loss, label_smoothing, stream_of(logits)),
        "xent_bwd_reg");
}

// ---- AdamW -------------------------------------------------------------------------------------
// Five entry points over three launchers. They share the helpers below; what each one asks of its
// tensors beyond that (dtypes, alignment) is checked in its own body.

// An optional device scalar of the AdamW kernels: `count` or more elements of T on p's device, else null.
template <typename T>
const T* adamw_dev_scalar(const char* what, const at::Tensor& p, const c10::optional<at::Tensor>& t, const char* name,
                          int64_t count) {
  if (!t.has_value()) return nullptr;
  constexpr at::ScalarType st = c10::CppTypeToScalarType<T>::value;
  TORCH_CHECK(t->scalar_type() == st && t->numel() >= count, what, ": ", name, " must be ", st, "[", count, "]");
  same_dev(p, *t, name);
  return t->data_ptr<T>();
}

// The launchers' argument block (kernels/launchers.h) from the scalars every entry point takes; sr stays
// zero (round to nearest). gscale_dev fp32[1], hyper_dev fp64[3] = {lr, bc1, bc2_sqrt}, skip_dev int32[1]
// (non-zero: the launch does nothing); each is optional.
pra_adamw_args adamw_args(const char* what, const at::Tensor& p, double lr, double b1, double b2, double eps,
                          double wd, double bc1, double bc2_sqrt, double gscale,
                          const c10::optional<at::Tensor>& gscale_dev, const c10::optional<at::Tensor>& hyper_dev,
                          bool fast, const c10::optional<at::Tensor>& skip_dev) {
  pra_adamw_args a{};
  a.lr = lr, a.b1 = b1, a.b2 = b2, a.eps = eps, a.wd = wd, a.bc1 = bc1, a.bc2_sqrt = bc2_sqrt;
  a.gscale = (float)gscale;
  a.fast = fast ? 1 : 0;
  a.gscale_dev = adamw_dev_scalar<float>(what, p, gscale_dev, "gscale_dev", 1);
  a.hyper_dev = adamw_dev_scalar<double>(what, p, hyper_dev, "hyper_dev", 3);
  a.skip_dev = adamw_dev_scalar<int>(what, p, skip_dev, "skip_dev", 1);
  return a;
}

// What the stochastic-rounding entry points add to the block (csrc/kernels/philox_sr.h).
pra_sr_args sr_args(const char* what, const at::Tensor& p, uint64_t seed, int64_t base, int64_t step,
                    const c10::optional<at::Tensor>& step_dev, int64_t mask) {
  TORCH_CHECK(p.scalar_type() == at::kBFloat16 || p.scalar_type() == at::kHalf, what,
              ": stochastic rounding needs bf16 or fp16 parameters and moments");
  TORCH_CHECK(base >= 0 && base % 8 == 0, what, ": base must be >= 0 and a multiple of 8, got ", base);
  TORCH_CHECK(mask >= 1 && mask <= 7, what, ": mask must be in 1..7, got ", mask);
  TORCH_CHECK(step >= 0 && step <= INT32_MAX, what, ": step");
  return pra_sr_args{seed, base, (int)step, adamw_dev_scalar<int>(what, p, step_dev, "step_dev", 1), (int)mask};
}

void check_aligned16(const char* what, std::initializer_list<at::Tensor> ts) {
  for (const at::Tensor& t : ts)
    TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, what, ": operands must be 16-B aligned");
}

// Flat p / g / m / v: contiguous, of one length, on p's device.
void check_adamw_flat(const char* what, const at::Tensor& p, const at::Tensor& g, const at::Tensor& m,
                      const at::Tensor& v) {
  check_dev(p, "p");
  TORCH_CHECK(p.is_contiguous() && g.is_contiguous() && m.is_contiguous() && v.is_contiguous(), what, ": contiguous");
  TORCH_CHECK(p.numel() == g.numel() && p.numel() == m.numel() && p.numel() == v.numel(), what, ": sizes");
  same_dev(p, g, "grad");
  same_dev(p, m, "exp_avg");
  same_dev(p, v, "exp_avg_sq");
}

// The tiled kernel's matrices: contiguous [rows, cols] p / g / m / v and pt [cols, rows] of p's dtype on p's
// device, rows and cols multiples of 64 (the tile), every pointer 16-B aligned (16-B loads and stores).
void check_adamw_t(const char* what, const at::Tensor& p, const at::Tensor& g, const at::Tensor& m,
                   const at::Tensor& v, const at::Tensor& pt) {
  check_dev(p, "p");
  TORCH_CHECK(p.dim() == 2 && p.is_contiguous() && g.sizes() == p.sizes() && m.sizes() == p.sizes() &&
                  v.sizes() == p.sizes() && g.is_contiguous() && m.is_contiguous() && v.is_contiguous(),
              what, ": p/g/m/v must be contiguous [rows, cols]");
  const int64_t rows = p.size(0), cols = p.size(1);
  TORCH_CHECK(pt.dim() == 2 && pt.size(0) == cols && pt.size(1) == rows && pt.is_contiguous(), what,
              ": pt [cols, rows]");
  TORCH_CHECK(rows % 64 == 0 && cols % 64 == 0, what, ": rows and cols must be multiples of 64");
  for (const at::Tensor& t : {g, m, v, pt}) {
    same_dev(p, t, "adamw_t operand");
    TORCH_CHECK(t.scalar_type() == p.scalar_type(), what, ": dtypes must match");
  }
  check_aligned16(what, {p, g, m, v, pt});
}

void adamw_flat_(at::Tensor p, const at::Tensor& g, at::Tensor m, at::Tensor v, double lr, double b1, double b2,
                 double eps, double wd, double bc1, double bc2_sqrt, double gscale,
                 const c10::optional<at::Tensor>& gscale_dev, const c10::optional<at::Tensor>& hyper_dev, bool fast,
                 const c10::optional<at::Tensor>& skip_dev) {
  const Range range_("pyrecover::adamw_flat");
  check_adamw_flat("adamw", p, g, m, v);
  TORCH_CHECK(g.scalar_type() == p.scalar_type() && m.scalar_type() == v.scalar_type(), "adamw: dtypes");
  const c10::DeviceGuard guard(p.device());
  const pra_adamw_args a =
      adamw_args("adamw", p, lr, b1, b2, eps, wd, bc1, bc2_sqrt, gscale, gscale_dev, hyper_dev, fast, skip_dev);
  check(pra_adamw_flat(dt(p), dt(m), p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), &a,
                       stream_of(p)),
        "adamw_flat");
}

// fp32-master AdamW: pm, m, v fp32; p (16-bit) <- round(pm); g has p's dtype.
void adamw_master_(at::Tensor p, at::Tensor pm, const at::Tensor& g, at::Tensor m, at::Tensor v, double lr, double b1,
                   double b2, double eps, double wd, double bc1, double bc2_sqrt, double gscale,
                   const c10::optional<at::Tensor>& gscale_dev, const c10::optional<at::Tensor>& hyper_dev, bool fast,
                   const c10::optional<at::Tensor>& skip_dev) {
  const Range range_("pyrecover::adamw_master");
  check_dev(p, "p");
  TORCH_CHECK(p.is_contiguous() && pm.is_contiguous() && g.is_contiguous() && m.is_contiguous() && v.is_contiguous(),
              "adamw_master: contiguous");
  TORCH_CHECK(p.numel() == pm.numel() && p.numel() == g.numel() && p.numel() == m.numel() && p.numel() == v.numel(),
              "adamw_master: sizes");
  TORCH_CHECK(p.element_size() == 2 && g.scalar_type() == p.scalar_type(), "adamw_master: 16-bit p and g");
  TORCH_CHECK(pm.scalar_type() == at::kFloat && m.scalar_type() == at::kFloat && v.scalar_type() == at::kFloat,
              "adamw_master: fp32 master and moments");
  for (const at::Tensor& t : {pm, g, m, v}) same_dev(p, t, "adamw_master operand");
  const c10::DeviceGuard guard(p.device());
  const pra_adamw_args a = adamw_args("adamw_master", p, lr, b1, b2, eps, wd, bc1, bc2_sqrt, gscale, gscale_dev,
                                      hyper_dev, fast, skip_dev);
  check(pra_adamw_master(dt(p), p.data_ptr(), pm.data_ptr<float>(), g.data_ptr(), m.data_ptr<float>(),
                         v.data_ptr<float>(), p.numel(), &a, stream_of(p)),
        "adamw_master");
}

// AdamW of one row-major weight matrix p [rows, cols] that also writes pt = p^T [cols, rows].
void adamw_t_(at::Tensor p, const at::Tensor& g, at::Tensor m, at::Tensor v, at::Tensor pt, double lr, double b1,
              double b2, double eps, double wd, double bc1, double bc2_sqrt, double gscale,
              const c10::optional<at::Tensor>& gscale_dev, const c10::optional<at::Tensor>& hyper_dev, bool fast,
              const c10::optional<at::Tensor>& skip_dev) {
  const Range range_("pyrecover::adamw_t");
  check_adamw_t("adamw_t", p, g, m, v, pt);
  TORCH_CHECK(p.element_size() == 2, "adamw_t: 16-bit parameters required");
  const c10::DeviceGuard guard(p.device());
  const pra_adamw_args a =
      adamw_args("adamw_t", p, lr, b1, b2, eps, wd, bc1, bc2_sqrt, gscale, gscale_dev, hyper_dev, fast, skip_dev);
  check(pra_adamw_t(dt(p), p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), pt.data_ptr(), (int)p.size(0),
                    (int)p.size(1), &a, stream_of(p)),
        "adamw_t");
}

// adamw_flat_ for 16-bit state with the tensors in `mask` (bit 0 p, 1 exp_avg, 2 exp_avg_sq) rounded
// stochastically; p[0] is flat position `base`, the step number is `step` or (when given) step_dev[0].
void adamw_flat_sr_(at::Tensor p, const at::Tensor& g, at::Tensor m, at::Tensor v, double lr, double b1, double b2,
                    double eps, double wd, double bc1, double bc2_sqrt, double gscale,
                    const c10::optional<at::Tensor>& gscale_dev, const c10::optional<at::Tensor>& hyper_dev, bool fast,
                    const c10::optional<at::Tensor>& skip_dev, uint64_t seed, int64_t base, int64_t step,
                    const c10::optional<at::Tensor>& step_dev, int64_t mask) {
  const Range range_("pyrecover::adamw_flat_sr");
  check_adamw_flat("adamw_sr", p, g, m, v);
  TORCH_CHECK(g.scalar_type() == p.scalar_type() && m.scalar_type() == p.scalar_type() &&
                  v.scalar_type() == p.scalar_type(), "adamw_sr: dtypes must match");
  const pra_sr_args sr = sr_args("adamw_flat_sr", p, seed, base, step, step_dev, mask);
  check_aligned16("adamw_flat_sr", {p, g, m, v});
  const c10::DeviceGuard guard(p.device());
  pra_adamw_args a =
      adamw_args("adamw_sr", p, lr, b1, b2, eps, wd, bc1, bc2_sqrt, gscale, gscale_dev, hyper_dev, fast, skip_dev);
  a.sr = sr;
  check(pra_adamw_flat(dt(p), dt(m), p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), &a,
                       stream_of(p)),
        "adamw_flat_sr");
}

// adamw_t_ with stochastic rounding; p[0][0] is flat position `base`, pt takes the rounded p.
void adamw_t_sr_(at::Tensor p, const at::Tensor& g, at::Tensor m, at::Tensor v, at::Tensor pt, double lr, double b1,
                 double b2, double eps, double wd, double bc1, double bc2_sqrt, double gscale,
                 const c10::optional<at::Tensor>& gscale_dev, const c10::optional<at::Tensor>& hyper_dev, bool fast,
                 const c10::optional<at::Tensor>& skip_dev, uint64_t seed, int64_t base, int64_t step,
                 const c10::optional<at::Tensor>& step_dev, int64_t mask) {
  const Range range_("pyrecover::adamw_t_sr");
  check_adamw_t("adamw_t_sr", p, g, m, v, pt);
  const pra_sr_args sr = sr_args("adamw_t_sr", p, seed, base, step, step_dev, mask);
  const c10::DeviceGuard guard(p.device());
  pra_adamw_args a =
      adamw_args("adamw_t_sr", p, lr, b1, b2, eps, wd, bc1, bc2_sqrt, gscale, gscale_dev, hyper_dev, fast, skip_dev);
  a.sr = sr;
  check(pra_adamw_t(dt(p), p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), pt.data_ptr(), (int)p.size(0),
                    (int)p.size(1), &a, stream_of(p)),
        "adamw_t_sr");
}

// dst = src^T for a 2-D 16-bit tensor (bf16/fp16) with R, C multiples of 64 (dst: optional
// preallocated [C, R] row-major output).
at::Tensor transpose2d(const at::Tensor& src, c10::optional<at::Tensor> out) {
  const Range range_("pyrecover::transpose2d");
  check_dev(src, "src");
  check_row_major(src, "src");
  TORCH_CHECK(src.element_size() == 2, "transpose2d: 16-bit dtype required");
  const int64_t R = src.size(0), C = src.size(1);
  TORCH_CHECK(R % 64 == 0 && C % 64 == 0 && src.stride(0) % 8 == 0, "transpose2d: R, C must be multiples of 64");
  const c10::DeviceGuard guard(src.device());
  at::Tensor dst;
  if (out.has_value()) {
    dst = *out;
    same_dev(src, dst, "out");
    check_row_major(dst, "out");
    TORCH_CHECK(dst.size(0) == C && dst.size(1) == R && dst.scalar_type() == src.scalar_type() &&
                    dst.stride(0) % 8 == 0,
                "transpose2d: out must be [C, R] of the same dtype");
  } else {
    dst = at::empty({C, R}, src.options());
  }
  check(pra_transpose16(src.data_ptr(), dst.data_ptr(), R, C, src.stride(0), dst.stride(0), stream_of(src)),
        "transpose2d");
  return dst;
}

// CU count of a tensor's device (cached per device)
int device_cus(const at::Tensor& t) {
  static int cached[64] = {0};
  const int d = t.device().index();
  if (d >= 0 && d < 64 && cached[d] > 0) return cached[d];
  int cus = 0;
  TORCH_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, d) == hipSuccess && cus > 0,
              "pyrecover_amd: device attribute");
  if (d >= 0 && d < 64) cached[d] = cus;
  return cus;
}

// What wgrad_mm_ and gemm_nt_ share. gemm_tensors: the operand checks that come before the op's own shape
// check. gemm_args: the dtype / dimension / stride checks, and the argument block with the three operands
// filled in. gemm_scratch: the split tail's fp32 partial tiles and tickets, sized by the plan the launcher
// runs (gemm_plan.h), from the caching allocator (graph-capture safe); none when the tiles fill whole rounds.
static void gemm_tensors(const at::Tensor& a, const at::Tensor& b, const at::Tensor& out) {
  check_dev(a, "a");
  check_row_major(a, "a");
  check_row_major(b, "b");
  check_row_major(out, "out");
  same_dev(a, b, "b");
  same_dev(a, out, "out");
}
static pra_gemm_args gemm_args(const char* op, const at::Tensor& a, const at::Tensor& b, const at::Tensor& out,
                               int64_t M, int64_t N, int64_t K) {
  TORCH_CHECK(a.scalar_type() == b.scalar_type() && a.scalar_type() == out.scalar_type() && a.element_size() == 2, op,
              ": bf16/fp16 operands of one dtype");
  TORCH_CHECK(M % 256 == 0 && N % 256 == 0 && K % 32 == 0 && K > 0, op, ": M, N % 256 and K % 32");
  TORCH_CHECK(a.stride(0) % 8 == 0 && b.stride(0) % 8 == 0 && out.stride(0) % 8 == 0, op, ": 16-B rows");
  pra_gemm_args g = {};
  g.dtype = dt(a);
  g.M = (int)M, g.N = (int)N, g.K = (int)K;
  g.a = a.data_ptr(), g.lda = a.stride(0);
  g.b = b.data_ptr(), g.ldb = b.stride(0);
  g.c = out.data_ptr(), g.ldc = out.stride(0);
  return g;
}
struct GemmScratch {
  at::Tensor ws, tickets;
};
static GemmScratch gemm_scratch(int kind, pra_gemm_args& g, const at::Tensor& a) {
  GemmScratch sc;
  g.cus = device_cus(a);
  long nws = 0;
  int ntk = 0;
  pra_gemm_scratch(kind, g.M, g.N, g.K, g.cus, &nws, &ntk);
  if (nws > 0) {
    sc.ws = at::empty({(int64_t)nws}, a.options().dtype(at::kFloat));
    sc.tickets = at::empty({(int64_t)ntk}, a.options().dtype(at::kInt));
    g.ws = sc.ws.data_ptr<float>();
    g.tickets = sc.tickets.data_ptr<int>();
  }
  return sc;
}

// out [M, N] (+)= a^T b with a [K, M], b [K, N] (both row-major, K = tokens): the weight gradient
// dW = dY^T X straight from the activations (no transposed copies), hand-written MFMA kernel.
void wgrad_mm_(const at::Tensor& a, const at::Tensor& b, at::Tensor out, bool accumulate) {
  const Range range_("pyrecover::wgrad_mm");
  gemm_tensors(a, b, out);
  const int64_t K = a.size(0), M = a.size(1), N = b.size(1);
  TORCH_CHECK(b.size(0) == K && out.size(0) == M && out.size(1) == N, "wgrad_mm: shapes [K,M] x [K,N] -> [M,N]");
  pra_gemm_args g = gemm_args("wgrad_mm", a, b, out, M, N, K);
  g.accumulate = accumulate ? 1 : 0;
  const c10::DeviceGuard guard(a.device());
  const GemmScratch sc = gemm_scratch(pra::kGemmWgrad, g, a);
  check(pra_wgrad_gemm(&g, stream_of(a)), "wgrad_mm");
}

// NT GEMM with a fused epilogue (gemm_nt.hip): a [M, K], b [N, K] row-major (K-contiguous).
//   epi 0: out [M, N] = a b^T
//   epi 1: SwiGLU forward, b = W1|W3 [2F, K]: out = gu [M, 2F], out2 = a [M, F]
//   epi 2: SwiGLU backward, b [F, K] (W2^T): da = a b^T is consumed in the epilogue, which
//          overwrites g, u in out = gu [M, 2F] with dg, du
//   epi 3: RoPE on the first nrot columns of out [M, N] (tab float32 [S, D/2, 2])
void gemm_nt_(const at::Tensor& a, const at::Tensor& b, at::Tensor out, int64_t epi,
              const c10::optional<at::Tensor>& out2, const c10::optional<at::Tensor>& tab, int64_t S, int64_t D,
              int64_t nrot) {
  const Range range_("pyrecover::gemm_nt");
  gemm_tensors(a, b, out);
  const int64_t M = a.size(0), K = a.size(1), N = b.size(0);
  TORCH_CHECK(b.size(1) == K, "gemm_nt: a [M, K] and b [N, K]");
  pra_gemm_args g = gemm_args("gemm_nt", a, b, out, M, N, K);
  TORCH_CHECK(reinterpret_cast<uintptr_t>(a.data_ptr()) % 16 == 0 && reinterpret_cast<uintptr_t>(b.data_ptr()) % 16 == 0 &&
                  reinterpret_cast<uintptr_t>(out.data_ptr()) % 16 == 0,
              "gemm_nt: 16-B aligned operands (the epilogue stores 16 B per lane)");
  TORCH_CHECK(epi >= 0 && epi <= 3, "gemm_nt: epi in 0..3");
  g.epi = (int)epi;
  g.S = (int)S, g.D = (int)D, g.nrot = (int)nrot;
  if (epi == 0 || epi == 3) {
    TORCH_CHECK(out.size(0) == M && out.size(1) == N, "gemm_nt: out [M, N]");
  }
  if (epi == 1) {
    const int64_t F = N / 2;
    TORCH_CHECK(N % 2 == 0 && F % 128 == 0, "gemm_nt swiglu: b = W1|W3 [2F, K], F % 128");
    TORCH_CHECK(out.size(0) == M && out.size(1) == N, "gemm_nt swiglu: gu [M, 2F]");
    TORCH_CHECK(out2.has_value(), "gemm_nt swiglu: needs out2 = a [M, F]");
    check_row_major(*out2, "out2");
    same_dev(a, *out2, "out2");
    TORCH_CHECK(out2->scalar_type() == a.scalar_type() && out2->size(0) == M && out2->size(1) == F &&
                    out2->stride(0) % 8 == 0,
                "gemm_nt swiglu: a [M, F]");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(out2->data_ptr()) % 16 == 0, "gemm_nt swiglu: 16-B aligned out2");
    g.F = (int)F;
    g.c2 = out2->data_ptr();
    g.ldc2 = out2->stride(0);
  }
  if (epi == 2) {
    g.F = (int)N;
    TORCH_CHECK(out.size(0) == M && out.size(1) == 2 * N, "gemm_nt swiglu bwd: gu [M, 2F] with b [F, K]");
  }
  if (epi == 3) {
    TORCH_CHECK(tab.has_value(), "gemm_nt rope: needs tab");
    same_dev(a, *tab, "tab");
    TORCH_CHECK(tab->scalar_type() == at::kFloat && tab->is_contiguous() && tab->numel() >= S * (D / 2) * 2,
                "gemm_nt rope: tab float32 [>= S, D/2, 2]");
    TORCH_CHECK(S > 0 && D > 0 && D % 8 == 0 && nrot % D == 0 && nrot <= N && M % S == 0,
                "gemm_nt rope: S, D % 8, nrot % D, tokens % S");
    g.tab = tab->data_ptr();
  }
  const c10::DeviceGuard guard(a.device());
  const GemmScratch sc = gemm_scratch(pra::kGemmNT, g, a);
  check(pra_gemm_nt(&g, stream_of(a)), "gemm_nt");
}

// returns fp32 [2] = {norm, clip_coef}
at::Tensor grad_norm(const at::Tensor& x, double max_norm, double pre_scale) {
  const Range range_("pyrecover::grad_norm");
  check_dev(x, "x");
  TORCH_CHECK(x.is_contiguous(), "grad_norm: contiguous");
  const c10::DeviceGuard guard(x.device());
  auto fo = x.options().dtype(at::kFloat);
  at::Tensor ws = at::empty({pra_sumsq_partials()}, fo), out = at::empty({2}, fo);
  check(pra_grad_norm(dt(x), x.data_ptr(), x.numel(), ws.data_ptr<float>(), out.data_ptr<float>(), (float)max_norm,
                      (float)pre_scale, stream_of(x)),
        "grad_norm");
  return out;
}

// Loss-scale / non-finite guard step (optim.hip guard_finish_kernel): the sum of squares of x, or the
// squared norm sq (fp64[1], sharded optimizer), decides the skip flag, the scale state, the gradient
// multiplier out[1] and the bias corrections hyper[1:3]. state int32[8], out fp32[2], hyper fp64[3].
void guard_step_(const c10::optional<at::Tensor>& x, const c10::optional<at::Tensor>& sq, at::Tensor state,
                 at::Tensor out, at::Tensor hyper, double max_norm, double pre_scale, bool dynamic, int64_t interval,
                 double b1, double b2) {
  const Range range_("pyrecover::guard_step");
  check_dev(state, "state");
  TORCH_CHECK(x.has_value() != sq.has_value(), "guard_step: exactly one of x and sq");
  TORCH_CHECK(state.scalar_type() == at::kInt && state.numel() >= 8 && state.is_contiguous(), "guard_step: state int32[8]");
  TORCH_CHECK(out.scalar_type() == at::kFloat && out.numel() >= 2 && out.is_contiguous(), "guard_step: out fp32[2]");
  TORCH_CHECK(hyper.scalar_type() == at::kDouble && hyper.numel() >= 3 && hyper.is_contiguous(),
              "guard_step: hyper fp64[3]");
  TORCH_CHECK(interval >= 1 && interval <= INT32_MAX, "guard_step: interval");
  same_dev(state, out, "out");
  same_dev(state, hyper, "hyper");
  const c10::DeviceGuard guard(state.device());
  const void* xp = nullptr;
  const double* sqp = nullptr;
  int xdt = 0;
  int64_t n = 0;
  if (x.has_value()) {
    TORCH_CHECK(x->is_contiguous(), "guard_step: contiguous");
    same_dev(state, *x, "x");
    xp = x->data_ptr();
    xdt = dt(*x);
    n = x->numel();
  } else {
    TORCH_CHECK(sq->scalar_type() == at::kDouble && sq->numel() >= 1, "guard_step: sq fp64[1]");
    same_dev(state, *sq, "sq");
    sqp = sq->data_ptr<double>();
  }
  at::Tensor ws = at::empty({pra_sumsq_partials()}, state.options().dtype(at::kFloat));
  check(pra_guard_step(xdt, xp, n, sqp, ws.data_ptr<float>(), state.data_ptr<int>(), out.data_ptr<float>(),
                       hyper.data_ptr<double>(), (float)max_norm, (float)pre_scale, dynamic ? 1 : 0, (int)interval, b1,
                       b2, stream_of(state)),
        "guard_step");
}

// replica checksum of a contiguous buffer: {fp64 sum of its elements, 64-bit word hash (int64 bits)}
std::vector<at::Tensor> checksum(const at::Tensor& x) {
  const Range range_("pyrecover::checksum");
  check_dev(x, "x");
  TORCH_CHECK(x.is_contiguous(), "checksum: contiguous");
  const c10::DeviceGuard guard(x.device());
  const int nb = pra_checksum_blocks();
  auto sum = at::empty({1}, x.options().dtype(at::kDouble)), hash = at::empty({1}, x.options().dtype(at::kLong));
  auto ws_s = at::empty({nb}, x.options().dtype(at::kDouble)), ws_h = at::empty({nb}, x.options().dtype(at::kLong));
  check(pra_checksum(dt(x), x.data_ptr(), x.numel() * x.element_size(), ws_s.data_ptr<double>(),
                     reinterpret_cast<unsigned long long*>(ws_h.data_ptr<int64_t>()), sum.data_ptr<double>(),
                     reinterpret_cast<unsigned long long*>(hash.data_ptr<int64_t>()), stream_of(x)),
        "checksum");
  return {sum, hash};
}

// q/k/v/o views [B, S, H, D] with stride(3)==1, stride(2)==D, stride(0)==S*stride(1).
void check_bshd(const at::Tensor& t, const char* name, int64_t B, int64_t S, int64_t H, int64_t D,
                at::ScalarType dtype) {
  TORCH_CHECK(t.dim() == 4 && t.size(0) == B && t.size(1) == S && t.size(2) == H && t.size(3) == D,
              "attention: ", name, " must be [B, S, H, D] = [", B, ", ", S, ", ", H, ", ", D, "], got ", t.sizes());
  TORCH_CHECK(t.stride(3) == 1 && t.stride(2) == D && (B == 1 || S == 1 || t.stride(0) == S * t.stride(1)),
              "attention: ", name, " must have token-major layout with contiguous heads, strides ", t.strides());
  TORCH_CHECK(t.scalar_type() == dtype, "attention: ", name, " must be ", dtype, " like q");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, "attention: ", name, " must be 16-B aligned");
}

void check_attn_dtype(const at::Tensor& q) {
  TORCH_CHECK(q.scalar_type() == at::kBFloat16 || q.scalar_type() == at::kHalf || q.scalar_type() == at::kFloat,
              "attention: the HIP kernels take bf16, fp16 or fp32 (got ", q.scalar_type(),
              "); fp64 models run the attention in torch (pyrecover_amd.ops.fused)");
}

// Sequences that do not tile (S % 64 forward, S % 128 backward) run on zero-padded copies of
// length round_up(S, 128). Causal attention is exact on the padding as is: a real query never
// sees a later (padded) key, and padded query rows carry dO = 0, so they add nothing to dK/dV.
// Non-causal attention passes the real length as the key bound `skv` (keys >= skv are masked).
constexpr int64_t kSeqPad = 128;
int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }
at::Tensor pad_seq(const at::Tensor& t, int64_t Sp) {  // t itself when it needs no padding
  if (t.size(1) == Sp) return t;
  at::Tensor out = at::zeros({t.size(0), Sp, t.size(2), t.size(3)}, t.options());
  out.narrow(1, 0, t.size(1)).copy_(t);
  return out;
}
// tile: 64 for the plain forward (fp32: 128), 128 for the document-masked forward and every backward
int64_t padded_len(int64_t S, int64_t tile) { return S % tile ? round_up(S, kSeqPad) : S; }

// doc_start [B, S] int32 of a packed batch (attention_docs.hip): checked, and for a sequence that does not
// tile, padded to Sp with the last document's start, so pad tokens continue the last document
// (device ops only: the step may be under graph capture).
void check_doc_start(const at::Tensor& q, const at::Tensor& ds, int64_t B, int64_t S, bool causal) {
  TORCH_CHECK(causal, "attention: doc_start implies causal attention");
  TORCH_CHECK(q.scalar_type() == at::kBFloat16 || q.scalar_type() == at::kHalf,
              "attention: the document-masked kernels take bf16 or fp16 (fp32 / fp64 run torch math in "
              "pyrecover_amd.ops.fused)");
  TORCH_CHECK(ds.scalar_type() == at::kInt && ds.dim() == 2 && ds.size(0) == B && ds.size(1) == S &&
                  ds.is_contiguous(), "attention: doc_start must be contiguous int32 [B, S]");
  same_dev(q, ds, "doc_start");
}
at::Tensor pad_doc_start(const at::Tensor& ds, int64_t Sp) {
  const int64_t B = ds.size(0), S = ds.size(1);
  if (S == Sp) return ds;
  at::Tensor out = at::empty({B, Sp}, ds.options());
  out.narrow(1, 0, S).copy_(ds);
  out.narrow(1, S, Sp - S).copy_(ds.narrow(1, S - 1, 1).expand({B, Sp - S}));
  return out;
}

// The forward's share of the argument block, from the (padded) tensors the kernels will see; skv is the
// real sequence length.
pra_attn_args attn_args(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v, const at::Tensor& o,
                        const at::Tensor& lse, const at::Tensor& doc_start, double scale, bool causal, int64_t skv) {
  pra_attn_args a = {};
  a.dtype = dt(q);
  a.B = (int)q.size(0), a.S = (int)q.size(1), a.Hq = (int)q.size(2), a.Hkv = (int)k.size(2), a.D = (int)q.size(3);
  a.skv = (int)skv;
  a.causal = causal ? 1 : 0;
  a.scale = (float)scale;
  a.q = q.data_ptr(), a.ldq = q.stride(1);
  a.k = k.data_ptr(), a.ldk = k.stride(1);
  a.v = v.data_ptr(), a.ldv = v.stride(1);
  a.o = o.data_ptr(), a.ldo = o.stride(1);
  a.lse = lse.data_ptr<float>();
  a.doc_start = doc_start.defined() ? doc_start.data_ptr<int>() : nullptr;
  return a;
}

std::vector<at::Tensor> attn_fwd(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v, double scale,
                                 bool causal, const c10::optional<at::Tensor>& doc_start) {
  const Range range_("pyrecover::attn_fwd");
  check_dev(q, "q");
  check_attn_dtype(q);
  const int64_t B = q.size(0), S = q.size(1), Hq = q.size(2), D = q.size(3), Hkv = k.size(2);
  check_bshd(q, "q", B, S, Hq, D, q.scalar_type());
  check_bshd(k, "k", B, S, Hkv, D, q.scalar_type());
  check_bshd(v, "v", B, S, Hkv, D, q.scalar_type());
  same_dev(q, k, "k");
  same_dev(q, v, "v");
  TORCH_CHECK(D == 64 || D == 128, "attention: head_dim must be 64 or 128");
  TORCH_CHECK(Hq % Hkv == 0, "attention: n_heads must be a multiple of n_kv_heads");
  TORCH_CHECK(S > 0 && (S % 64 == 0 || S <= (int64_t)INT32_MAX - kSeqPad), "attention: bad seq_len");
  const c10::DeviceGuard guard(q.device());
  const bool docs = doc_start.has_value();  // packed sequences: document-masked kernels (128-row blocks)
  if (docs) check_doc_start(q, *doc_start, B, S, causal);
  // fp32 kernel: 128-query blocks
  const int64_t Sp = padded_len(S, docs || q.scalar_type() == at::kFloat ? kSeqPad : 64);
  const at::Tensor qp = pad_seq(q, Sp), kp = pad_seq(k, Sp), vp = pad_seq(v, Sp);
  const at::Tensor dsp = docs ? pad_doc_start(*doc_start, Sp) : at::Tensor();
  at::Tensor o = at::empty({B, Sp, Hq, D}, q.options());
  at::Tensor lse = at::empty({B, Hq, Sp}, q.options().dtype(at::kFloat));
  const pra_attn_args a = attn_args(qp, kp, vp, o, lse, dsp, scale, causal, S);
  check(pra_attn_fwd(&a, stream_of(q)), docs ? "attn_docs_fwd" : "attn_fwd");
  if (Sp != S) return {o.narrow(1, 0, S).contiguous(), lse.narrow(2, 0, S).contiguous()};
  return {o, lse};
}

// ---------------------------------------------------------------------------------------
// KV-cache generation (csrc/kernels/attention_decode.hip)
void check_decode_common(const at::Tensor& ref, const at::Tensor& kc, const at::Tensor& vc, const at::Tensor& kv_len,
                         int64_t B, const char* op) {
  TORCH_CHECK(ref.scalar_type() == at::kBFloat16 || ref.scalar_type() == at::kHalf, op,
              ": the HIP kernels take bf16 or fp16 (got ", ref.scalar_type(),
              "); other dtypes run the torch math of pyrecover_amd.ops.reference");
  same_dev(ref, kc, "k_cache");
  same_dev(ref, vc, "v_cache");
  same_dev(ref, kv_len, "kv_len");
  TORCH_CHECK(kc.dim() == 4 && kc.size(0) == B && kc.size(1) > 0 && kc.size(2) > 0, op,
              ": k_cache must be [B, cap, Hkv, D] with B = ", B, ", got ", kc.sizes());
  TORCH_CHECK(vc.sizes() == kc.sizes(), op, ": v_cache must have k_cache's shape");
  TORCH_CHECK(kc.is_contiguous() && vc.is_contiguous(), op, ": the caches must be contiguous");
  TORCH_CHECK(kc.scalar_type() == ref.scalar_type() && vc.scalar_type() == ref.scalar_type(), op,
              ": the caches must have the query's dtype");
  TORCH_CHECK(kc.size(3) == 64 || kc.size(3) == 128, op, ": head_dim must be 64 or 128");
  TORCH_CHECK(kc.size(1) <= (int64_t)INT32_MAX / 2 && kc.size(2) <= 65535 && B > 0 && B <= 65535, op, ": bad shape");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(kc.data_ptr()) % 16 == 0 && reinterpret_cast<uintptr_t>(vc.data_ptr()) % 16 == 0,
              op, ": the caches must be 16-B aligned");
  TORCH_CHECK(kv_len.scalar_type() == at::kInt && kv_len.dim() == 1 && kv_len.size(0) == B && kv_len.is_contiguous(),
              op, ": kv_len must be contiguous int32 [B]");
}

// qkv [B * T, (Hq + 2 Hkv) D] (rows of the fused QKV activation, T new tokens per sequence, B the caches'):
// row b * T + t has q rotated in place at position kv_len[b] + t, rotated k and plain v written into that
// row of the caches. T = 1 clamps the row to cap - 1; T > 1 stores nothing for a position >= cap.
void rope_append_(at::Tensor qkv, const at::Tensor& tab, const at::Tensor& kv_len, at::Tensor k_cache,
                  at::Tensor v_cache) {
  const Range range_("pyrecover::rope_append");
  check_dev(qkv, "qkv");
  check_row_major(qkv, "rope_append qkv");
  const int64_t B = k_cache.dim() == 4 ? k_cache.size(0) : qkv.size(0);
  check_decode_common(qkv, k_cache, v_cache, kv_len, B, "rope_append");
  const int64_t cap = k_cache.size(1), Hkv = k_cache.size(2), D = k_cache.size(3);
  TORCH_CHECK(qkv.size(0) > 0 && qkv.size(0) % B == 0 && qkv.size(0) / B <= (int64_t)INT32_MAX / 2,
              "rope_append: qkv must hold T rows for each of the caches' B = ", B, " sequences, got ", qkv.sizes());
  const int64_t T = qkv.size(0) / B;
  TORCH_CHECK(qkv.size(1) % D == 0 && qkv.size(1) / D > 2 * Hkv && (qkv.size(1) / D - 2 * Hkv) % Hkv == 0,
              "rope_append: qkv must be [B, (Hq + 2 Hkv) D] with Hq a multiple of Hkv, got ", qkv.sizes());
  TORCH_CHECK(qkv.stride(0) % 8 == 0, "rope_append: the qkv row stride must be a multiple of 8 elements");
  const int64_t Hq = qkv.size(1) / D - 2 * Hkv;
  same_dev(qkv, tab, "rope table");
  TORCH_CHECK(tab.scalar_type() == at::kFloat && tab.is_contiguous() && tab.dim() == 3 && tab.size(0) >= cap &&
                  tab.size(1) == D / 2 && tab.size(2) == 2,
              "rope_append: table must be contiguous fp32 [>= cap, D/2, 2]");
  const c10::DeviceGuard guard(qkv.device());
  check(pra_rope_append(dt(qkv), qkv.data_ptr(), tab.data_ptr(), kv_len.data_ptr<int>(), k_cache.data_ptr(),
                        v_cache.data_ptr(), (int)B, (int)T, qkv.stride(0), (int)Hq, (int)Hkv, (int)D, (int)cap,
                        stream_of(qkv)),
        "rope_append");
}

// q [B, T, Hq, D] (token rows may be strided views of the QKV activation), caches [B, cap, Hkv, D] that hold
// the T new tokens already, kv_len int32 [B] on the device (tokens held before this append)
// -> (o [B, T, Hq, D], lse fp32 [B, T, Hq]). Query t attends to keys 0 .. min(kv_len[b] + t, cap - 1).
std::vector<at::Tensor> attn_extend(const at::Tensor& q, const at::Tensor& k_cache, const at::Tensor& v_cache,
                                    const at::Tensor& kv_len, double scale) {
  const Range range_("pyrecover::attn_extend");
  check_dev(q, "q");
  TORCH_CHECK(q.dim() == 4 && q.size(1) > 0, "attn_extend: q must be [B, T, Hq, D], got ", q.sizes());
  const int64_t B = q.size(0), T = q.size(1), Hq = q.size(2), D = q.size(3);
  check_decode_common(q, k_cache, v_cache, kv_len, B, "attn_extend");
  const int64_t cap = k_cache.size(1), Hkv = k_cache.size(2);
  TORCH_CHECK(k_cache.size(3) == D, "attn_extend: q and the caches disagree on head_dim");
  TORCH_CHECK(Hq > 0 && Hq <= 65535 && Hq % Hkv == 0, "attn_extend: n_heads must be a multiple of n_kv_heads");
  TORCH_CHECK(T * (Hq / Hkv) <= (int64_t)INT32_MAX / 2, "attn_extend: bad shape");
  // rows of one token contiguous, tokens at one stride across the batch: else a packed copy
  int64_t ldq = T > 1 ? q.stride(1) : B > 1 ? q.stride(0) : Hq * D;  // a dim of size 1 has no stride to speak of
  const bool view_ok = q.stride(3) == 1 && q.stride(2) == D && ldq % 8 == 0 && ldq >= Hq * D &&
                       (B == 1 || q.stride(0) == T * ldq);
  at::Tensor qc = view_ok ? q : q.contiguous();
  if (!view_ok) ldq = Hq * D;
  TORCH_CHECK(reinterpret_cast<uintptr_t>(qc.data_ptr()) % 16 == 0, "attn_extend: q must be 16-B aligned");
  const c10::DeviceGuard guard(q.device());
  at::Tensor o = at::empty({B, T, Hq, D}, q.options());
  at::Tensor lse = at::empty({B, T, Hq}, q.options().dtype(at::kFloat));
  check(pra_attn_extend(dt(q), qc.data_ptr(), ldq, k_cache.data_ptr(), v_cache.data_ptr(),
                        kv_len.data_ptr<int>(), o.data_ptr(), lse.data_ptr<float>(), (int)B, (int)T, (int)Hq, (int)Hkv,
                        (int)D, (int)cap, (float)scale, stream_of(q)),
        "attn_extend");
  return {o, lse};
}

// q [B, Hq, D] (rows may be strided views of the QKV activation), caches [B, cap, Hkv, D], kv_len int32 [B]
// on the device -> (o [B, Hq, D], lse fp32 [B, Hq]).
std::vector<at::Tensor> attn_decode(const at::Tensor& q, const at::Tensor& k_cache, const at::Tensor& v_cache,
                                    const at::Tensor& kv_len, double scale) {
  const Range range_("pyrecover::attn_decode");
  check_dev(q, "q");
  TORCH_CHECK(q.dim() == 3, "attn_decode: q must be [B, Hq, D], got ", q.sizes());
  const int64_t B = q.size(0), Hq = q.size(1), D = q.size(2);
  check_decode_common(q, k_cache, v_cache, kv_len, B, "attn_decode");
  const int64_t cap = k_cache.size(1), Hkv = k_cache.size(2);
  TORCH_CHECK(k_cache.size(3) == D, "attn_decode: q and the caches disagree on head_dim");
  TORCH_CHECK(Hq > 0 && Hq <= 65535 && Hq % Hkv == 0, "attn_decode: n_heads must be a multiple of n_kv_heads");
  at::Tensor qc = q.contiguous();
  TORCH_CHECK(reinterpret_cast<uintptr_t>(qc.data_ptr()) % 16 == 0, "attn_decode: q must be 16-B aligned");
  const c10::DeviceGuard guard(q.device());
  at::Tensor o = at::empty({B, Hq, D}, q.options());
  at::Tensor lse = at::empty({B, Hq}, q.options().dtype(at::kFloat));
  at::Tensor ws = at::empty({pra_attn_decode_ws_floats((int)B, (int)Hq, (int)D, (int)cap)},
                            q.options().dtype(at::kFloat));
  check(pra_attn_decode(dt(q), qc.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), kv_len.data_ptr<int>(),
                        o.data_ptr(), lse.data_ptr<float>(), ws.data_ptr<float>(), (int)B, (int)Hq, (int)Hkv, (int)D,
                        (int)cap, (float)scale, stream_of(q)),
        "attn_decode");
  return {o, lse};
}

// fp8 KV cache (csrc/kernels/attention_decode_fp8.hip): the checks of check_decode_common with uint8 caches
// [B, cap, Hkv, D] of e4m3fn bytes and fp32 scales [B, cap, Hkv]. kv_len: absent for the prefill store.
void check_decode_fp8_common(const at::Tensor& ref, const at::Tensor& kc, const at::Tensor& vc, const at::Tensor& ks,
                             const at::Tensor& vs, const at::Tensor* kv_len, int64_t B, const char* op) {
  TORCH_CHECK(ref.scalar_type() == at::kBFloat16 || ref.scalar_type() == at::kHalf, op,
              ": the HIP kernels take bf16 or fp16 (got ", ref.scalar_type(),
              "); other dtypes run the torch math of pyrecover_amd.ops.reference");
  same_dev(ref, kc, "k_cache");
  same_dev(ref, vc, "v_cache");
  same_dev(ref, ks, "k_scale");
  same_dev(ref, vs, "v_scale");
  TORCH_CHECK(kc.dim() == 4 && kc.size(0) == B && kc.size(1) > 0 && kc.size(2) > 0, op,
              ": k_cache must be [B, cap, Hkv, D] with B = ", B, ", got ", kc.sizes());
  TORCH_CHECK(vc.sizes() == kc.sizes(), op, ": v_cache must have k_cache's shape");
  TORCH_CHECK(kc.is_contiguous() && vc.is_contiguous(), op, ": the caches must be contiguous");
  TORCH_CHECK(kc.scalar_type() == at::kByte && vc.scalar_type() == at::kByte, op,
              ": the fp8 caches must have dtype uint8 (e4m3fn bytes)");
  TORCH_CHECK(kc.size(3) == 64 || kc.size(3) == 128, op, ": head_dim must be 64 or 128");
  TORCH_CHECK(kc.size(1) <= (int64_t)INT32_MAX / 2 && kc.size(2) <= 65535 && B > 0 && B <= 65535, op, ": bad shape");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(kc.data_ptr()) % 16 == 0 && reinterpret_cast<uintptr_t>(vc.data_ptr()) % 16 == 0,
              op, ": the caches must be 16-B aligned");
  for (const at::Tensor* s : {&ks, &vs})
    TORCH_CHECK(s->scalar_type() == at::kFloat && s->dim() == 3 && s->size(0) == B && s->size(1) == kc.size(1) &&
                    s->size(2) == kc.size(2) && s->is_contiguous(),
                op, ": k_scale and v_scale must be contiguous fp32 [B, cap, Hkv], got ", s->sizes());
  if (kv_len != nullptr) {
    same_dev(ref, *kv_len, "kv_len");
    TORCH_CHECK(kv_len->scalar_type() == at::kInt && kv_len->dim() == 1 && kv_len->size(0) == B &&
                    kv_len->is_contiguous(),
                op, ": kv_len must be contiguous int32 [B]");
  }
}

// k, v [B, S, Hkv, D]: the k and v views of the fused QKV activation [B * S, ld] (or any tensors with that
// stride pattern) quantized into rows 0 .. S - 1 of the fp8 caches.
void kv_quantize_(const at::Tensor& k, const at::Tensor& v, at::Tensor k_cache, at::Tensor v_cache, at::Tensor k_scale,
                  at::Tensor v_scale) {
  const Range range_("pyrecover::kv_quantize");
  check_dev(k, "k");
  TORCH_CHECK(k.dim() == 4, "kv_quantize: k must be [B, S, Hkv, D], got ", k.sizes());
  const int64_t B = k.size(0), S = k.size(1), Hkv = k.size(2), D = k.size(3);
  check_decode_fp8_common(k, k_cache, v_cache, k_scale, v_scale, nullptr, B, "kv_quantize");
  same_dev(k, v, "v");
  TORCH_CHECK(v.sizes() == k.sizes() && v.scalar_type() == k.scalar_type() && v.strides() == k.strides(),
              "kv_quantize: v must have k's shape, dtype and strides");
  TORCH_CHECK(k_cache.size(2) == Hkv && k_cache.size(3) == D, "kv_quantize: k and the caches disagree on [Hkv, D]");
  TORCH_CHECK(S > 0 && S <= k_cache.size(1), "kv_quantize: ", S, " rows do not fit the cache capacity ", k_cache.size(1));
  const int64_t ld = k.stride(1);
  TORCH_CHECK(k.stride(3) == 1 && k.stride(2) == D && ld >= Hkv * D && ld % 8 == 0 && (B == 1 || k.stride(0) == S * ld),
              "kv_quantize: k and v must be [B, S, Hkv, D] views of rows [B * S, ld] with ld a multiple of 8 elements");
  TORCH_CHECK(B * S <= (int64_t)INT32_MAX / 2, "kv_quantize: bad shape");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(k.data_ptr()) % 16 == 0 && reinterpret_cast<uintptr_t>(v.data_ptr()) % 16 == 0,
              "kv_quantize: k and v must be 16-B aligned");
  const c10::DeviceGuard guard(k.device());
  check(pra_kv_quantize(dt(k), k.data_ptr(), v.data_ptr(), ld, k_cache.data_ptr(), v_cache.data_ptr(),
                        k_scale.data_ptr<float>(), v_scale.data_ptr<float>(), (int)B, (int)S, (int)Hkv, (int)D,
                        (int)k_cache.size(1), stream_of(k)),
        "kv_quantize");
}

// rope_append_ over an fp8 cache: q rotated in place (bit-equal), the rotated k row rounded to qkv's dtype and
// the plain v row quantized into cache row clamp(kv_len[b], 0, cap - 1).
void rope_append_fp8_(at::Tensor qkv, const at::Tensor& tab, const at::Tensor& kv_len, at::Tensor k_cache,
                      at::Tensor v_cache, at::Tensor k_scale, at::Tensor v_scale) {
  const Range range_("pyrecover::rope_append_fp8");
  check_dev(qkv, "qkv");
  check_row_major(qkv, "rope_append_fp8 qkv");
  const int64_t B = qkv.size(0);
  check_decode_fp8_common(qkv, k_cache, v_cache, k_scale, v_scale, &kv_len, B, "rope_append_fp8");
  const int64_t cap = k_cache.size(1), Hkv = k_cache.size(2), D = k_cache.size(3);
  TORCH_CHECK(qkv.size(1) % D == 0 && qkv.size(1) / D > 2 * Hkv && (qkv.size(1) / D - 2 * Hkv) % Hkv == 0,
              "rope_append_fp8: qkv must be [B, (Hq + 2 Hkv) D] with Hq a multiple of Hkv, got ", qkv.sizes());
  TORCH_CHECK(qkv.stride(0) % 8 == 0, "rope_append_fp8: the qkv row stride must be a multiple of 8 elements");
  const int64_t Hq = qkv.size(1) / D - 2 * Hkv;
  same_dev(qkv, tab, "rope table");
  TORCH_CHECK(tab.scalar_type() == at::kFloat && tab.is_contiguous() && tab.dim() == 3 && tab.size(0) >= cap &&
                  tab.size(1) == D / 2 && tab.size(2) == 2,
              "rope_append_fp8: table must be contiguous fp32 [>= cap, D/2, 2]");
  const c10::DeviceGuard guard(qkv.device());
  check(pra_rope_append_fp8(dt(qkv), qkv.data_ptr(), tab.data_ptr(), kv_len.data_ptr<int>(), k_cache.data_ptr(),
                            v_cache.data_ptr(), k_scale.data_ptr<float>(), v_scale.data_ptr<float>(), (int)B,
                            qkv.stride(0), (int)Hq, (int)Hkv, (int)D, (int)cap, stream_of(qkv)),
        "rope_append_fp8");
}

// attn_decode over an fp8 cache -> (o [B, Hq, D] in q's dtype, lse fp32 [B, Hq]).
std::vector<at::Tensor> attn_decode_fp8(const at::Tensor& q, const at::Tensor& k_cache, const at::Tensor& v_cache,
                                        const at::Tensor& k_scale, const at::Tensor& v_scale, const at::Tensor& kv_len,
                                        double scale) {
  const Range range_("pyrecover::attn_decode_fp8");
  check_dev(q, "q");
  TORCH_CHECK(q.dim() == 3, "attn_decode_fp8: q must be [B, Hq, D], got ", q.sizes());
  const int64_t B = q.size(0), Hq = q.size(1), D = q.size(2);
  check_decode_fp8_common(q, k_cache, v_cache, k_scale, v_scale, &kv_len, B, "attn_decode_fp8");
  const int64_t cap = k_cache.size(1), Hkv = k_cache.size(2);
  TORCH_CHECK(k_cache.size(3) == D, "attn_decode_fp8: q and the caches disagree on head_dim");
  TORCH_CHECK(Hq > 0 && Hq <= 65535 && Hq % Hkv == 0, "attn_decode_fp8: n_heads must be a multiple of n_kv_heads");
  at::Tensor qc = q.contiguous();
  TORCH_CHECK(reinterpret_cast<uintptr_t>(qc.data_ptr()) % 16 == 0, "attn_decode_fp8: q must be 16-B aligned");
  const c10::DeviceGuard guard(q.device());
  at::Tensor o = at::empty({B, Hq, D}, q.options());
  at::Tensor lse = at::empty({B, Hq}, q.options().dtype(at::kFloat));
  at::Tensor ws = at::empty({pra_attn_decode_ws_floats((int)B, (int)Hq, (int)D, (int)cap)},
                            q.options().dtype(at::kFloat));
  check(pra_attn_decode_fp8(dt(q), qc.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), k_scale.data_ptr<float>(),
                            v_scale.data_ptr<float>(), kv_len.data_ptr<int>(), o.data_ptr(), lse.data_ptr<float>(),
                            ws.data_ptr<float>(), (int)B, (int)Hq, (int)Hkv, (int)D, (int)cap, (float)scale,
                            stream_of(q)),
        "attn_decode_fp8");
  return {o, lse};
}

// Device-side sampling (csrc/kernels/sample.hip): logits [B, V] bf16 / fp16 (row stride >= V) -> tok int64 [B].
// temperature 0 is greedy; otherwise pos (int32 [B]) or, with the generation state, prompt_len + count
// indexes the Philox draw. ws: int32 workspace of sample_ws_bytes(B) bytes (allocated here when absent).
// The generation state (done uint8, count / room int32 [B], out int64 [B, max_new]) is given whole or not
// at all.
void sample_(const at::Tensor& logits, at::Tensor tok, double temperature, int64_t top_k, double top_p, int64_t seed,
             const c10::optional<at::Tensor>& pos, c10::optional<at::Tensor> ws, c10::optional<at::Tensor> u_out,
             c10::optional<at::Tensor> done, c10::optional<at::Tensor> count, const c10::optional<at::Tensor>& room,
             c10::optional<at::Tensor> out, int64_t eos_id, const c10::optional<at::Tensor>& prompt_len) {
  const Range range_("pyrecover::sample");
  check_dev(logits, "logits");
  TORCH_CHECK(logits.scalar_type() == at::kBFloat16 || logits.scalar_type() == at::kHalf,
              "sample: the HIP kernel takes bf16 or fp16 logits (got ", logits.scalar_type(),
              "); other dtypes run pyrecover_amd.ops.reference.sample_philox_ref");
  TORCH_CHECK(logits.dim() == 2 && logits.size(0) > 0 && logits.size(1) > 0, "sample: logits must be [B, V], got ",
              logits.sizes());
  const int64_t B = logits.size(0), V = logits.size(1);
  TORCH_CHECK(B <= 65535 && V <= (int64_t(1) << 30), "sample: B <= 65535 and V <= 2^30");
  TORCH_CHECK((V == 1 || logits.stride(1) == 1) && (B == 1 || logits.stride(0) >= V),
              "sample: logits need unit inner stride and a row stride >= V");
  const int64_t ld = B == 1 ? V : logits.stride(0);
  TORCH_CHECK(temperature >= 0.0 && temperature <= 3.0e38, "sample: temperature must be finite and >= 0, got ",
              temperature);
  TORCH_CHECK(top_p > 0.0 && top_p <= 1.0, "sample: top_p must be in (0, 1], got ", top_p);
  TORCH_CHECK(top_k >= 0 && top_k <= INT32_MAX, "sample: top_k must be >= 0, got ", top_k);
  auto vec = [&](const at::Tensor& t, at::ScalarType ty, const char* name) {
    same_dev(logits, t, name);
    TORCH_CHECK(t.scalar_type() == ty && t.dim() == 1 && t.size(0) == B && t.is_contiguous(), "sample: ", name,
                " must be contiguous ", ty, " [B]");
  };
  vec(tok, at::kLong, "tok");
  pra_sample_args a = {};
  a.temperature = (float)temperature;
  a.top_k = (int)top_k;
  a.top_p = (float)top_p;
  TORCH_CHECK(temperature == 0.0 || a.temperature > 0.f, "sample: temperature underflows fp32");
  TORCH_CHECK(a.top_p > 0.f, "sample: top_p underflows fp32");
  a.seed = (unsigned long long)seed;
  a.tok = (long long*)tok.data_ptr<int64_t>();
  const bool stateful = done.has_value();
  TORCH_CHECK(count.has_value() == stateful && room.has_value() == stateful && out.has_value() == stateful,
              "sample: done, count, room and out are given together or not at all");
  TORCH_CHECK(stateful || !prompt_len.has_value(), "sample: prompt_len needs the generation state");
  if (stateful) {
    vec(*done, at::kByte, "done");
    vec(*count, at::kInt, "count");
    vec(*room, at::kInt, "room");
    same_dev(logits, *out, "out");
    TORCH_CHECK(out->scalar_type() == at::kLong && out->dim() == 2 && out->size(0) == B && out->size(1) > 0 &&
                    out->size(1) <= INT32_MAX && out->is_contiguous(),
                "sample: out must be contiguous int64 [B, max_new]");
    a.gen.done = done->data_ptr<uint8_t>();
    a.gen.count = count->data_ptr<int>();
    a.gen.room = room->data_ptr<int>();
    a.gen.out = (long long*)out->data_ptr<int64_t>();
    a.gen.max_new = (int)out->size(1);
    a.gen.eos_id = eos_id;
    if (prompt_len.has_value()) {
      vec(*prompt_len, at::kInt, "prompt_len");
      a.gen.prompt_len = prompt_len->data_ptr<int>();
    }
  }
  const c10::DeviceGuard guard(logits.device());
  if (temperature > 0.0) {
    TORCH_CHECK(pos.has_value() || prompt_len.has_value(), "sample: a draw needs pos (or prompt_len with the state)");
    if (pos.has_value()) {
      vec(*pos, at::kInt, "pos");
      a.pos = pos->data_ptr<int>();
    }
    const int64_t need = pra_sample_ws_bytes((int)B);
    if (!ws.has_value()) ws = at::empty({need / 4}, logits.options().dtype(at::kInt));
    same_dev(logits, *ws, "ws");
    TORCH_CHECK(ws->scalar_type() == at::kInt && ws->is_contiguous() && ws->numel() * 4 >= need &&
                    reinterpret_cast<uintptr_t>(ws->data_ptr()) % 16 == 0,
                "sample: ws must be contiguous, 16-B aligned int32 with at least ", need, " bytes");
    a.ws = (unsigned*)ws->data_ptr<int>();
    if (u_out.has_value()) {
      vec(*u_out, at::kFloat, "u_out");
      a.u_out = u_out->data_ptr<float>();
    }
  }
  check(pra_sample(dt(logits), logits.data_ptr(), ld, (int)B, (int)V, &a, stream_of(logits)), "sample");
}

// Writes dq/dk/dv into caller-provided [B,S,H,D] views (e.g. slices of a fused dQKV buffer).
void attn_bwd(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v, const at::Tensor& o,
              const at::Tensor& dout, const at::Tensor& lse, at::Tensor dq, at::Tensor dk, at::Tensor dv, double scale,
              bool causal, c10::optional<at::Tensor> rope_tab, int64_t mid_event,
              const c10::optional<at::Tensor>& doc_start) {
  const Range range_("pyrecover::attn_bwd");
  // mid_event (optional, a torch.cuda.Event's cuda_event handle): recorded on the stream between the
  // dQ and dK/dV kernels, so another stream can start work under the dK/dV kernel
  hipEvent_t mev = reinterpret_cast<hipEvent_t>(mid_event);
  check_dev(q, "q");
  check_attn_dtype(q);
  const int64_t B = q.size(0), S = q.size(1), Hq = q.size(2), D = q.size(3), Hkv = k.size(2);
  const at::ScalarType ty = q.scalar_type();
  const std::tuple<const at::Tensor&, const char*, int64_t> operands[] = {
      {q, "q", Hq}, {k, "k", Hkv}, {v, "v", Hkv}, {o, "o", Hq}, {dout, "dout", Hq}, {dq, "dq", Hq}, {dk, "dk", Hkv},
      {dv, "dv", Hkv}};
  for (const auto& [t, name, H] : operands) check_bshd(t, name, B, S, H, D, ty);
  TORCH_CHECK(D == 64 || D == 128, "attention: head_dim must be 64 or 128");
  TORCH_CHECK(Hq % Hkv == 0, "attention: n_heads must be a multiple of n_kv_heads");
  TORCH_CHECK(lse.scalar_type() == at::kFloat && lse.numel() == B * Hq * S && lse.is_contiguous(), "attention: lse");
  for (const at::Tensor& t : {k, v, o, dout, lse, dq, dk, dv}) same_dev(q, t, "attention operand");
  // optional RoPE table [>= S, D/2, 2] fp32 (cos, sin): dq / dk are stored with the inverse rotation
  const float* rtab = nullptr;
  if (rope_tab.has_value()) {
    TORCH_CHECK(ty != at::kFloat, "attention: the fp32 backward has no fused inverse RoPE (pass rope_tab=None)");
    const at::Tensor& tb = *rope_tab;
    TORCH_CHECK(tb.scalar_type() == at::kFloat && tb.is_contiguous() && tb.numel() >= S * D &&
                    tb.numel() % D == 0, "attention: rope table must be contiguous fp32 [>= S, D/2, 2]");
    same_dev(q, tb, "rope table");
    rtab = tb.data_ptr<float>();
  }
  const c10::DeviceGuard guard(q.device());
  const bool docs = doc_start.has_value();  // packed sequences: document-masked kernels
  if (docs) check_doc_start(q, *doc_start, B, S, causal);
  const int64_t Sp = padded_len(S, kSeqPad);
  const bool pad = Sp != S;
  const at::Tensor qp = pad_seq(q, Sp), kp = pad_seq(k, Sp), vp = pad_seq(v, Sp), op = pad_seq(o, Sp),
                   dop = pad_seq(dout, Sp);
  const at::Tensor dsp = docs ? pad_doc_start(*doc_start, Sp) : at::Tensor();
  at::Tensor lp = lse, dqp = dq, dkp = dk, dvp = dv;
  if (pad) {
    lp = at::zeros({B, Hq, Sp}, lse.options());  // padded rows: any finite lse (their dO is zero)
    lp.narrow(2, 0, S).copy_(lse.view({B, Hq, S}));
    dqp = at::empty_like(qp), dkp = at::empty_like(kp), dvp = at::empty_like(vp);
  }
  pra_attn_args a = attn_args(qp, kp, vp, op, lp, dsp, scale, causal, S);
  a.dout = dop.data_ptr(), a.lddo = dop.stride(1);
  a.dq = dqp.data_ptr(), a.lddq = dqp.stride(1);
  a.dk = dkp.data_ptr(), a.lddk = dkp.stride(1);
  a.dv = dvp.data_ptr(), a.lddv = dvp.stride(1);
  a.rope_tab = rtab;
  a.mid_event = mev;
  at::Tensor ws = at::empty({pra_attn_bwd_workspace(&a)}, q.options().dtype(at::kFloat));
  a.ws = ws.data_ptr<float>();
  check(pra_attn_bwd(&a, stream_of(q)), docs ? "attn_docs_bwd" : "attn_bwd");
  if (pad) {
    dq.copy_(dqp.narrow(1, 0, S));
    dk.copy_(dkp.narrow(1, 0, S));
    dv.copy_(dvp.narrow(1, 0, S));
  }
}

}  // namespace

void register_ckpt_engine(pybind11::module& m);  // csrc/runtime/ckpt_engine.cpp
void register_xgmi(pybind11::module& m);         // csrc/comm/xgmi.cpp

PYBIND11_MODULE(_C, m) {
  m.doc() = "pyrecover_amd native ops (HIP/gfx950 kernels + checkpoint engine)";
  m.def("set_roctx", [](bool on) { g_roctx.store(on); });
  m.def("roctx_enabled", []() { return g_roctx.load(); });
  m.def("rmsnorm_fwd", &rmsnorm_fwd);
  m.def("rmsnorm_bwd", &rmsnorm_bwd);
  m.def("layernorm_fwd", &layernorm_fwd);
  m.def("layernorm_bwd", &layernorm_bwd);
  m.def("rope_", &rope_, pybind11::arg("x2d"), pybind11::arg("ncols"), pybind11::arg("tab"),
        pybind11::arg("head_dim"), pybind11::arg("seq_len"), pybind11::arg("pos_offset"), pybind11::arg("inverse"),
        pybind11::arg("doc_start") = pybind11::none());
  m.def("swiglu_fwd", &swiglu_fwd);
  m.def("swiglu_bwd", &swiglu_bwd, pybind11::arg("dy"), pybind11::arg("gu"), pybind11::arg("out") = pybind11::none(),
        pybind11::arg("variant") = -1);
  m.def("embedding_fwd", &embedding_fwd);
  m.def("embedding_bwd", &embedding_bwd);
  m.def("xent_fwd", &xent_fwd);
  m.def("xent_bwd_", &xent_bwd_);
  m.def("xent_fwd_reg", &xent_fwd_reg);
  m.def("xent_bwd_reg_", &xent_bwd_reg_);
  namespace py = pybind11;
  // the scalars every AdamW entry point takes after its tensors, and what the stochastic-rounding ones add
#define PRA_ADAMW_PYARGS                                                                                          \
  py::arg("lr"), py::arg("b1"), py::arg("b2"), py::arg("eps"), py::arg("wd"), py::arg("bc1"), py::arg("bc2_sqrt"), \
      py::arg("gscale"), py::arg("gscale_dev") = py::none(), py::arg("hyper_dev") = py::none(),                   \
      py::arg("fast") = false, py::arg("skip_dev") = py::none()
#define PRA_ADAMW_SR_PYARGS \
  py::kw_only(), py::arg("seed"), py::arg("base"), py::arg("step"), py::arg("step_dev") = py::none(), py::arg("mask")
  m.def("adamw_flat_", &adamw_flat_, py::arg("p"), py::arg("g"), py::arg("m"), py::arg("v"), PRA_ADAMW_PYARGS);
  m.def("adamw_t_", &adamw_t_, py::arg("p"), py::arg("g"), py::arg("m"), py::arg("v"), py::arg("pt"),
        PRA_ADAMW_PYARGS);
  m.def("adamw_flat_sr_", &adamw_flat_sr_, py::arg("p"), py::arg("g"), py::arg("m"), py::arg("v"), PRA_ADAMW_PYARGS,
        PRA_ADAMW_SR_PYARGS);
  m.def("adamw_t_sr_", &adamw_t_sr_, py::arg("p"), py::arg("g"), py::arg("m"), py::arg("v"), py::arg("pt"),
        PRA_ADAMW_PYARGS, PRA_ADAMW_SR_PYARGS);
  m.def("adamw_master_", &adamw_master_, py::arg("p"), py::arg("pm"), py::arg("g"), py::arg("m"), py::arg("v"),
        PRA_ADAMW_PYARGS);
#undef PRA_ADAMW_PYARGS
#undef PRA_ADAMW_SR_PYARGS
  m.def("grad_norm", &grad_norm);
  m.def("guard_step_", &guard_step_, py::arg("x"), py::arg("sq"), py::arg("state"), py::arg("out"), py::arg("hyper"),
        py::arg("max_norm"), py::arg("pre_scale"), py::arg("dynamic"), py::arg("interval"), py::arg("b1"),
        py::arg("b2"));
  m.def("checksum", &checksum);
  m.def("wgrad_mm_", &wgrad_mm_);
  m.def("gemm_nt_", &gemm_nt_, py::arg("a"), py::arg("b"), py::arg("out"), py::arg("epi") = 0,
        py::arg("out2") = py::none(), py::arg("tab") = py::none(), py::arg("S") = 0, py::arg("D") = 0,
        py::arg("nrot") = 0);
  m.def("transpose2d", &transpose2d, py::arg("src"), py::arg("out") = py::none());
  m.def("swiglu_bwd_t_", &swiglu_bwd_t_);
  m.def("swiglu_fwd_t", &swiglu_fwd_t);
  m.def("rope_t_", &rope_t_);
  m.def("attn_fwd", &attn_fwd, pybind11::arg("q"), pybind11::arg("k"), pybind11::arg("v"), pybind11::arg("scale"),
        pybind11::arg("causal"), pybind11::arg("doc_start") = pybind11::none());
  m.def("attn_bwd", &attn_bwd, pybind11::arg("q"), pybind11::arg("k"), pybind11::arg("v"), pybind11::arg("o"),
        pybind11::arg("dout"), pybind11::arg("lse"), pybind11::arg("dq"), pybind11::arg("dk"), pybind11::arg("dv"),
        pybind11::arg("scale"), pybind11::arg("causal"), pybind11::arg("rope_tab") = pybind11::none(),
        pybind11::arg("mid_event") = 0, pybind11::arg("doc_start") = pybind11::none());
  m.def("rope_append_", &rope_append_, py::arg("qkv"), py::arg("tab"), py::arg("kv_len"), py::arg("k_cache"),
        py::arg("v_cache"));
  m.def("attn_decode", &attn_decode, py::arg("q"), py::arg("k_cache"), py::arg("v_cache"), py::arg("kv_len"),
        py::arg("scale"));
  m.def("attn_decode_chunk", []() { return pra_attn_decode_chunk(); });
  m.def("attn_extend", &attn_extend, py::arg("q"), py::arg("k_cache"), py::arg("v_cache"), py::arg("kv_len"),
        py::arg("scale"));
  m.def("kv_quantize_", &kv_quantize_, py::arg("k"), py::arg("v"), py::arg("k_cache"), py::arg("v_cache"),
        py::arg("k_scale"), py::arg("v_scale"));
  m.def("rope_append_fp8_", &rope_append_fp8_, py::arg("qkv"), py::arg("tab"), py::arg("kv_len"), py::arg("k_cache"),
        py::arg("v_cache"), py::arg("k_scale"), py::arg("v_scale"));
  m.def("attn_decode_fp8", &attn_decode_fp8, py::arg("q"), py::arg("k_cache"), py::arg("v_cache"), py::arg("k_scale"),
        py::arg("v_scale"), py::arg("kv_len"), py::arg("scale"));
  m.def("attn_decode_fp8_chunk", []() { return pra_attn_decode_fp8_chunk(); });
  m.def("sample_", &sample_, py::arg("logits"), py::arg("tok"), py::arg("temperature"), py::arg("top_k"),
        py::arg("top_p"), py::arg("seed"), py::arg("pos") = py::none(), py::arg("ws") = py::none(),
        py::arg("u_out") = py::none(), py::arg("done") = py::none(), py::arg("count") = py::none(),
        py::arg("room") = py::none(), py::arg("out") = py::none(), py::arg("eos_id") = -1,
        py::arg("prompt_len") = py::none());
  m.def("sample_ws_bytes", [](int B) { return pra_sample_ws_bytes(B); });
  // every field of pra_attn_options (csrc/kernels/attn_plan.h documents them), by keyword
  m.def("attn_set_options", [](int fwd_pipe, double fwd_thr, int dkdv_impl, int dq_pipe, int dkdv_split, int dkdv_kreg,
                               int bwd_fused, int bwd_window, int fwd_order, int dq_order, int dkdv_order) {
    const pra_attn_options o = {fwd_pipe,  (float)fwd_thr, dkdv_impl, dq_pipe,  dkdv_split, dkdv_kreg,
                                bwd_fused, bwd_window,     fwd_order, dq_order, dkdv_order};
    pra_attn_set_options(&o);
  }, py::kw_only(), py::arg("fwd_pipe"), py::arg("fwd_thr"), py::arg("dkdv_impl"), py::arg("dq_pipe"),
     py::arg("dkdv_split"), py::arg("dkdv_kreg"), py::arg("bwd_fused"), py::arg("bwd_window"), py::arg("fwd_order"),
     py::arg("dq_order"), py::arg("dkdv_order"));
  register_ckpt_engine(m);
  register_xgmi(m);
}
