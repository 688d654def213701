// The rank-1 expand family's one arithmetic.  expand1d_e4m3_kernel,
// expand1d_bf16_e4m3_kernel and expand1d_bf16_e5m2_kernel (gemm_mx8.hip) are
// thin shells over these pieces, so an output two of them produce is the same
// bits by construction.  expand1d_kernel (mlp_small.hip) writes the same
// statements out in its own loop (it measured slower built from the pieces,
// profiles/shared_tile_epilogue.md); the tests compare it with them bitwise.
// All four op wrappers share expand1d_args below.
//
// out[row, 8*c8 + e] = act(x[row] * w[8*c8 + e] + b[8*c8 + e]) [* mask bit];
// one thread per (row, c8): 8 columns = one 16-byte bf16 store.  A 1-bit
// ReLU mask is uint8 [n, H/8], bit e of byte c8 = column 8*c8+e > 0.
#pragma once
#include <hip/hip_runtime.h>
#include <torch/extension.h>

#include "bf16_utils.h"

// grid-stride loop over the first n rows: f(row, c8) for every 8-column chunk
template <class F>
__device__ __forceinline__ void e1d_for_each_chunk(long long n, int h8, F f) {
  const long long total = (long long)n * h8;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
       idx < total; idx += stride)
    f(idx / h8, (int)(idx % h8));
}

// element offset of chunk (row, c8) in an [n, H] output
__device__ __forceinline__ long long e1d_offset(long long row, int h8, int c8) {
  return row * (long long)h8 * 8 + c8 * 8;
}

// acc[e] = x*w[e] (+ b[e]), then relu
template <bool RELU, bool HAS_BIAS>
__device__ __forceinline__ void e1d_axpb(float xv,
                                         const bf16_t* __restrict__ w,
                                         const bf16_t* __restrict__ b, int c8,
                                         float (&acc)[8]) {
  float wv[8], bv[8];
  bf16x8_to_f32(load_bf16x8(w + c8 * 8), wv);
  if (HAS_BIAS) bf16x8_to_f32(load_bf16x8(b + c8 * 8), bv);
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    acc[e] = HAS_BIAS ? fmaf(xv, wv[e], bv[e]) : xv * wv[e];
    if (RELU) acc[e] = fmaxf(acc[e], 0.0f);
  }
}

__device__ __forceinline__ void e1d_apply_mask(unsigned char mb,
                                               float (&acc)[8]) {
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = (mb >> e) & 1 ? acc[e] : 0.0f;
}

__device__ __forceinline__ unsigned char e1d_mask_bits(const float (&acc)[8]) {
  unsigned char mb = 0;
#pragma unroll
  for (int e = 0; e < 8; ++e) mb |= (acc[e] > 0.0f ? 1u : 0u) << e;
  return mb;
}

// RNE to bf16, one 16-byte store; returns what was stored
__device__ __forceinline__ bf16x8 e1d_store_bf16(bf16_t* __restrict__ out,
                                                 long long o,
                                                 const float (&acc)[8]) {
  const bf16x8 ob = f32_to_bf16x8(acc);
  store_bf16x8(out + o, ob);
  return ob;
}

// 8 values -> 8 e4m3 bytes (value = stored / inv_scale), one 8-byte store.
// The HW packed convert rounds to nearest-even.
__device__ __forceinline__ void e1d_store_e4m3(
    unsigned char* __restrict__ out8, long long o, const float (&acc)[8],
    float inv_scale) {
  unsigned long long packed = 0;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    unsigned int pk = (unsigned int)__builtin_amdgcn_cvt_pk_fp8_f32(
        acc[2 * p] * inv_scale, acc[2 * p + 1] * inv_scale, 0, false);
    packed |= (unsigned long long)(pk & 0xFFFFu) << (16 * p);
  }
  *(unsigned long long*)(out8 + o) = packed;
}

// OCP e5m2 (S.EEEEE.MM, bias 15, max finite 57344, inf at 0x7C), the
// gradient format.  The scaled value is clamped to +-57344 in plain code
// BEFORE the packed convert, so saturation is defined here and never by the
// instruction's overflow mode; NaN passes through the comparisons unchanged.
__device__ __forceinline__ float mx_e5m2_prescale(float v, int e) {
  v = ldexpf(v, -e);  // exact power-of-two scaling for any e in [-127,127]
  v = v > 57344.0f ? 57344.0f : v;
  v = v < -57344.0f ? -57344.0f : v;
  return v;
}

// two floats -> two e5m2 bytes (RNE) in the low 16 bits
__device__ __forceinline__ unsigned int mx_cvt2_e5m2(float v0, float v1) {
  return (unsigned int)__builtin_amdgcn_cvt_pk_bf8_f32(v0, v1, 0, false) &
         0xFFFFu;
}

// 8 values -> 8 e5m2 bytes (value = 2^e * stored), one 8-byte store
__device__ __forceinline__ void e1d_store_e5m2(
    unsigned char* __restrict__ out8, long long o, const float (&v)[8],
    int e) {
  unsigned long long packed = 0;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    unsigned int pk = mx_cvt2_e5m2(mx_e5m2_prescale(v[2 * p], e),
                                   mx_e5m2_prescale(v[2 * p + 1], e));
    packed |= (unsigned long long)pk << (16 * p);
  }
  *(unsigned long long*)(out8 + o) = packed;
}

// ---- host side: what the four op wrappers check and compute alike ----------
struct Expand1dArgs {
  long long n = 0, H = 0;
  int h8 = 0;    // H / 8
  int grid = 0;  // blocks of 256 threads
  const float* x = nullptr;
  const bf16_t* w = nullptr;
  const bf16_t* b = nullptr;  // nullptr: no bias
};

static inline Expand1dArgs expand1d_args(const char* op, const at::Tensor& x,
                                         const at::Tensor& w,
                                         const c10::optional<at::Tensor>& b) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kFloat, op,
              ": x must be an fp32 cuda tensor");
  TORCH_CHECK(w.scalar_type() == at::kBFloat16, op, ": w must be bf16");
  Expand1dArgs a;
  a.n = x.numel();
  a.H = w.numel();
  TORCH_CHECK(a.H % 8 == 0, op, ": H must be a multiple of 8");
  a.h8 = (int)(a.H / 8);
  if (b.has_value()) {
    TORCH_CHECK(b->scalar_type() == at::kBFloat16 && b->numel() == a.H, op,
                ": bias must be bf16 [H]");
    a.b = (const bf16_t*)b->data_ptr();
  }
  a.grid = (int)std::min<long long>((a.n * a.h8 + 255) / 256, 2048);
  a.x = x.data_ptr<float>();
  a.w = (const bf16_t*)w.data_ptr();
  return a;
}
