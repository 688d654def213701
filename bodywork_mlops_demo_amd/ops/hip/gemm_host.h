// Host side of the GEMM ops (gemm.hip, gemm8.hip, gemm_mx8.hip,
// gemm_mx4.hip): the operand check and launch record of the 256x256-tile
// kernels, the runtime -> template epilogue ladder and the quantisers'
// launch.  Device code is in tile256.h (front end) and mfma_tile.h (epilogue).
#pragma once
#include <hip/hip_runtime.h>
#include <torch/extension.h>

#include <algorithm>
#include <type_traits>

#include "host_checks.h"
#include "mfma_tile.h"

// gemm8.hip's launcher, called from gemm.hip's dispatch
void launch_gemm8(Epi epi, bool has_bias, bool out_fp32, bool emit_mask,
                  const void* ap, const void* bp, const float* bias,
                  const unsigned char* mask, unsigned char* mask_out,
                  void* cp, long long M, long long N, long long K);

// optional fp32 [N] epilogue vector (bias, b2, w3) -> pointer, nullptr
// when absent
static inline const float* epi_vec_n(const char* op, const char* what,
                                     const c10::optional<at::Tensor>& v,
                                     long long N) {
  if (!v.has_value() || !v->defined()) return nullptr;
  TORCH_CHECK(v->is_cuda() && v->scalar_type() == torch::kFloat &&
                  v->numel() == N && v->is_contiguous(),
              op, ": ", what, " must be a contiguous fp32 [N] cuda tensor");
  return v->data_ptr<float>();
}

// ---- operands of a 256x256-tile kernel --------------------------------------

// How an operand format stores K: elements of `dtype`, kbytes_num/kbytes_den
// bytes per K element (fp4: 1/2), K a multiple of k_mult.  k_max (0: none)
// keeps a kernel's 32-bit per-lane staging offset in range.
struct GemmFormat {
  at::ScalarType dtype;
  const char* dtype_text;
  int kbytes_num, kbytes_den;
  int k_mult;
  long long k_max;
};

// The problem and operand pointers of one launch; an op's record adds what
// its kernel takes beyond them.
struct GemmOperands {
  long long M = 0, N = 0, K = 0;
  const void* a = nullptr;
  const void* b = nullptr;
  bool empty() const { return M == 0 || N == 0; }  // nothing to launch
  dim3 grid() const { return dim3((unsigned)(N / 256), (unsigned)(M / 256)); }
};

// The operand pair every 256x256-tile op takes: a [M, K] and b [N, K] in
// format f, both K-major.  `op` prefixes the error texts.
static inline GemmOperands gemm256_operands(const char* op, const GemmFormat& f,
                                            const at::Tensor& a,
                                            const at::Tensor& b) {
  TORCH_CHECK(a.is_cuda() && b.is_cuda() && a.device() == b.device(), op,
              ": operands must be cuda tensors on one device");
  TORCH_CHECK(a.scalar_type() == f.dtype && b.scalar_type() == f.dtype, op,
              ": operands must be ", f.dtype_text, " tensors");
  TORCH_CHECK(a.dim() == 2 && b.dim() == 2 && a.size(1) == b.size(1), op,
              ": [M,K]x[N,K] operands (", f.kbytes_num, "/", f.kbytes_den,
              " bytes per K element)");
  TORCH_CHECK(a.is_contiguous() && b.is_contiguous(), op,
              ": operands must be contiguous");
  GemmOperands g;
  g.M = a.size(0), g.N = b.size(0);
  g.K = a.size(1) * (long long)a.element_size() * f.kbytes_den / f.kbytes_num;
  TORCH_CHECK(g.M % 256 == 0 && g.N % 256 == 0 && g.K % f.k_mult == 0, op,
              " requires M%256==0, N%256==0, K%", f.k_mult, "==0 (got ", g.M,
              "x", g.N, "x", g.K, ")");
  TORCH_CHECK(f.k_max == 0 || g.K <= f.k_max, op, ": K too large");
  TORCH_CHECK((uintptr_t)a.data_ptr() % 16 == 0 &&
                  (uintptr_t)b.data_ptr() % 16 == 0,
              op, ": operands must be 16-byte aligned");
  g.a = a.data_ptr();
  g.b = b.data_ptr();
  return g;
}

// Everything a block-scaled kernel launch (gemm_mx8_nt_1p_kernel,
// gemm_mxfp4_nt_kernel) takes.  Each op sets the scales and the epilogue
// pointers it uses and leaves the rest null.
struct MxGemm : GemmOperands {
  explicit MxGemm(const GemmOperands& o) : GemmOperands(o) {}
  const unsigned char* a8() const { return (const unsigned char*)a; }
  const unsigned char* b8() const { return (const unsigned char*)b; }
  int sa = 127, sb = 127;             // fp8: per-tensor E8M0 bytes (host part)
  const int* ea_dev = nullptr;        // fp8 DEV_SCALE
  const int* eb_dev = nullptr;
  const unsigned char* sa_blk = nullptr;  // fp4: block scale tensors
  const unsigned char* sb_blk = nullptr;
  const float* bias = nullptr;        // BiasRelu / ReluDot
  const float* w3 = nullptr;          // ReluDot
  unsigned char* mask_out = nullptr;  // EMIT_MASK
  const unsigned char* mask_in = nullptr;  // MaskMul
  const int64_t* n_live = nullptr;         // LIVE
  void* c = nullptr;
};

// ---- epilogue ladder --------------------------------------------------------

template <Epi E>
using EpiTag = std::integral_constant<Epi, E>;

// Runtime (relu, has_bias, out_fp32) -> f(EpiTag, has_bias tag, out_fp32 tag),
// the six-way None / BiasRelu family; f is a generic lambda that reads each
// tag's ::value as a template argument.  Without relu there is no bias.
template <class F>
static inline void dispatch_epilogue(bool relu, bool has_bias, bool out_fp32,
                                     F&& f) {
  auto out = [&](auto epi, auto hb) {
    if (out_fp32) f(epi, hb, std::true_type{});
    else          f(epi, hb, std::false_type{});
  };
  if (!relu)         out(EpiTag<Epi::None>{}, std::false_type{});
  else if (has_bias) out(EpiTag<Epi::BiasRelu>{}, std::true_type{});
  else               out(EpiTag<Epi::BiasRelu>{}, std::false_type{});
}

// ---- quantiser launch -------------------------------------------------------

// x is bf16 or fp32 (checked here); `work` items, one per thread, grid-stride
// past 8192 blocks of 256.  launch(xp, blocks) gets x's data as const short*
// (bf16) or const float*, and is not called when there is no work.
template <class F>
static inline void launch_quantiser(const char* op, const at::Tensor& x,
                                    long long work, F&& launch) {
  const bool bf16 = x.scalar_type() == torch::kBFloat16;
  TORCH_CHECK(bf16 || x.scalar_type() == torch::kFloat, op,
              ": bf16 or fp32 input");
  if (work == 0) return;
  const int blocks = (int)std::min<long long>((work + 255) / 256, 8192);
  if (bf16) launch((const short*)x.data_ptr(), blocks);
  else      launch((const float*)x.data_ptr(), blocks);
}
