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

// ---- MXFP4: OCP e2m1 codes, one E8M0 scale per 32 consecutive K elements ---
//
// The scale bytes of an [R, K] operand (R % 64 == 0, K % 256 == 0) are stored
// in the order gemm_mx4.hip's K-loop reads them: per (64-row group G, 256-
// element K-tile t) one 512-byte chunk, lane-major, so a wave fetches the
// scales of its 64 rows for one K-tile with ONE coalesced 8-byte load per
// lane.  Lane kg*16+fl owns the 8 bytes [h][i] = scale of row 16*i+fl of the
// group, 32-block 4*h+kg of the tile: dword h is the scale VGPR of the K=128
// MFMA h, and the fragment index i is its op_sel byte.
// ops/reference.py (mxfp4_scale_index) mirrors this rule.
__device__ __forceinline__ long long mx4_scale_index(long long row, int blk,
                                                     int nt /* K/256 */) {
  const long long G = row >> 6;
  const int r = (int)(row & 63);
  const int t = blk >> 3, b = blk & 7;
  return ((G * nt + t) * 64 + (b & 3) * 16 + (r & 15)) * 8 + (b >> 2) * 4 +
         (r >> 4);
}

// Block exponent from |amax|'s bit pattern: the smallest e with amax / 2^e
// <= 6 (= 1.5 * 2^2), clamped to [-127, 127]; 0 for a zero or non-finite
// amax.  Field arithmetic, so the boundary is exact.
__device__ __forceinline__ int mx4_block_exponent(unsigned int amax_bits) {
  const int E = (int)(amax_bits >> 23);
  const unsigned int man = amax_bits & 0x7FFFFFu;
  if (amax_bits == 0u || E == 255) return 0;
  const int e = E - 127 - 2 + (man > 0x400000u ? 1 : 0);
  return min(max(e, -127), 127);
}

// The quantiser's arithmetic on 8 values of one thread, shared by
// e1d_store_mxfp4 below and by the skinny fp4 forward (mlp_skinny_mx4.hip),
// which quantises in registers: what both emit is the same bits by
// construction.  mx4_amax8: the largest |value| bit pattern (monotone as
// unsigned ints; NaN and inf sort on top).  mx4_pack8: the 8 e2m1 codes at
// block exponent e, element 2i in the low nibble of byte i; values are scaled
// exactly (ldexpf) and converted at unit scale by the packed RNE convert,
// which saturates at +-6.
__device__ __forceinline__ unsigned int mx4_amax8(const float (&acc)[8]) {
  unsigned int am = 0u;
#pragma unroll
  for (int e = 0; e < 8; ++e)
    am = max(am, __float_as_uint(acc[e]) & 0x7FFFFFFFu);
  return am;
}

__device__ __forceinline__ unsigned int mx4_pack8(const float (&acc)[8],
                                                  int e) {
  float v[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] = ldexpf(acc[k], -e);
  unsigned int pk = 0u;
  pk = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(pk, v[0], v[1], 1.0f, 0);
  pk = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(pk, v[2], v[3], 1.0f, 1);
  pk = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(pk, v[4], v[5], 1.0f, 2);
  pk = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(pk, v[6], v[7], 1.0f, 3);
  return pk;
}

// 8 values of one thread -> 8 e2m1 codes (one 4-byte store, element 2i in the
// low nibble of byte i) and, from the first of the four ADJACENT lanes that
// hold a 32-block, its E8M0 byte.  The block amax is two cross-lane steps
// over the four lanes' mx4_amax8.  Every lane of such a group of four must
// be active: callers iterate (row, c8) with c8 fastest and H/8 a multiple of
// 4.
__device__ __forceinline__ void e1d_store_mxfp4(
    unsigned char* __restrict__ q, unsigned char* __restrict__ s,
    long long row, int h8, int c8, const float (&acc)[8]) {
  unsigned int am = mx4_amax8(acc);
  am = max(am, (unsigned int)__shfl_xor((int)am, 1, 64));
  am = max(am, (unsigned int)__shfl_xor((int)am, 2, 64));
  const int e = mx4_block_exponent(am);
  const unsigned int pk = mx4_pack8(acc, e);
  *(unsigned int*)(q + ((row * h8 + c8) << 2)) = pk;
  if ((c8 & 3) == 0)
    s[mx4_scale_index(row, c8 >> 2, h8 >> 5)] = (unsigned char)(e + 127);
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
