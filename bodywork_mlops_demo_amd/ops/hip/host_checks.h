// Host-side argument checks shared by the op wrappers.
#pragma once
#include <torch/extension.h>

// optional int64[1] live row count on the operand's device -> pointer
// (nullptr when absent or undefined).  `op` prefixes the error text.
static inline const int64_t* n_live_ptr(
    const c10::optional<at::Tensor>& n_dev, const at::Tensor& like,
    const char* op) {
  if (!n_dev.has_value() || !n_dev->defined()) return nullptr;
  TORCH_CHECK(n_dev->is_cuda() && n_dev->device() == like.device() &&
                  n_dev->numel() == 1 && n_dev->scalar_type() == at::kLong,
              op, ": n_dev must be an int64[1] tensor on the operand's device");
  return n_dev->data_ptr<int64_t>();
}

// ---- the one-kernel MLP scoring forwards (mlp_skinny.hip, mlp_mid.hip) ------

// a contiguous [numel] tensor of `dtype` on x's device -> its data pointer
static inline const void* mlp_score_operand(const char* op, const char* name,
                                            const at::Tensor& t,
                                            const at::Tensor& x,
                                            at::ScalarType dtype,
                                            int64_t numel) {
  TORCH_CHECK(t.is_cuda() && t.device() == x.device() &&
                  t.scalar_type() == dtype && t.numel() == numel &&
                  t.is_contiguous(),
              op, ": ", name, " must be a contiguous ", c10::toString(dtype),
              " tensor of ", numel, " elements on x's device");
  return t.data_ptr();
}

// what the host entries check alike: x fp32 [1..max_m], H = w1.numel() a
// multiple of k_chunk; w1, b1 (and a bf16 w2) are bf16
struct MlpScoreOperands {
  int64_t m = 0, H = 0;
  const void *w1 = nullptr, *b1 = nullptr, *w2 = nullptr;
  const float *b2 = nullptr, *w3 = nullptr, *b3 = nullptr;
};

// everything but w2, whose format is the kernel's (mlp_skinny_mx4.hip takes
// MXFP4 codes and scales)
static inline MlpScoreOperands mlp_score_vectors(
    const char* op, int64_t max_m, int64_t k_chunk, const at::Tensor& x,
    const at::Tensor& w1, const at::Tensor& b1, const at::Tensor& b2,
    const at::Tensor& w3, const at::Tensor& b3) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kFloat && x.dim() == 1 &&
                  x.is_contiguous(),
              op, ": x must be a contiguous 1-d fp32 cuda tensor");
  MlpScoreOperands a;
  a.m = x.numel();
  TORCH_CHECK(a.m >= 1 && a.m <= max_m, op, ": serves 1..", max_m,
              " rows (got ", a.m, ")");
  const int64_t H = a.H = w1.numel();
  TORCH_CHECK(H > 0 && H % k_chunk == 0 && H <= (1 << 20), op,
              ": H must be a positive multiple of ", k_chunk,
              ", at most 2^20 (got ", H, ")");
  a.w1 = mlp_score_operand(op, "w1", w1, x, at::kBFloat16, H);
  a.b1 = mlp_score_operand(op, "b1", b1, x, at::kBFloat16, H);
  a.b2 = (const float*)mlp_score_operand(op, "b2", b2, x, at::kFloat, H);
  a.w3 = (const float*)mlp_score_operand(op, "w3", w3, x, at::kFloat, H);
  a.b3 = (const float*)mlp_score_operand(op, "b3", b3, x, at::kFloat, 1);
  return a;
}

static inline MlpScoreOperands mlp_score_operands(
    const char* op, int64_t max_m, int64_t k_chunk, const at::Tensor& x,
    const at::Tensor& w1, const at::Tensor& b1, const at::Tensor& w2,
    const at::Tensor& b2, const at::Tensor& w3, const at::Tensor& b3) {
  MlpScoreOperands a =
      mlp_score_vectors(op, max_m, k_chunk, x, w1, b1, b2, w3, b3);
  TORCH_CHECK(w2.dim() == 2 && w2.size(0) == a.H && w2.size(1) == a.H, op,
              ": w2 must be [H, H] = [out, in]");
  a.w2 = mlp_score_operand(op, "w2", w2, x, at::kBFloat16, a.H * a.H);
  return a;
}
