// Device side of drift_histograms (drift_hist.hip) — gfx950.
//
// THE SLOT RULE.  A histogram row k has bins equal cells over [lo_k, hi_k)
// and bins + 3 slots.  For a value v, with scale_k = fp32(bins) /
// (fp32(hi_k) - fp32(lo_k)) computed once in Python and passed down:
//   t = __fmul_rn(__fsub_rn(v, lo_k), scale_k)
//   slot = bins + 2      (NaN)        if t != t
//        = 0             (underflow)  else if t < 0
//        = bins + 1      (overflow)   else if t >= bins
//        = 1 + (int)t                 otherwise
// so +inf is overflow, -inf underflow and inf - inf NaN.  The residual row
// bins __fsub_rn(label, score).  Every step is a single correctly rounded
// fp32 operation (no FMA contraction), which ops/reference.py mirrors in
// numpy float32; the counts are integers, so the result is exact, bitwise
// reproducible and independent of the grid.
//
// Stage 1 (drift_hist_kernel): float4 body + scalar tail, grid-stride; each
// wave adds into its own LDS copy of the 4 x (bins + 3) table with
// no-return LDS integer adds (one add of the lane count when the whole wave
// agrees on the slot); after a barrier the block folds its waves' copies
// and writes them with plain stores into row blockIdx.x of a
// [grid, 4 * (bins + 3)] uint32 workspace.  Stage 2 (drift_hist_finalize):
// sums the workspace rows into int64, consecutive threads on consecutive
// groups of four slots.  No global atomics.  The host passes the grid; a
// block must see fewer than 2^32 rows.
#pragma once
#include <hip/hip_runtime.h>

#include "lds_hist.h"  // DH_BLOCK, dh_add, drift_hist_finalize

#define DH_MAX_BINS 256
#define DH_ROWS 4  // x, labels, scores, labels - scores

struct DriftBins {
  float lo[DH_ROWS];
  float scale[DH_ROWS];
};

__device__ __forceinline__ int dh_slot(float v, float lo, float scale,
                                       int bins) {
  const float t = __fmul_rn(__fsub_rn(v, lo), scale);
  // the conversion is used only where 0 <= t < bins
  int s = 1 + (int)t;
  s = t >= (float)bins ? bins + 1 : s;
  s = t < 0.f ? 0 : s;
  s = t != t ? bins + 2 : s;
  return s;
}

// one input row into the wave's table `my` ([DH_ROWS][S], S = bins + 3)
__device__ __forceinline__ void dh_row(unsigned int* my, int S, int bins,
                                       const DriftBins& p, float x, float l,
                                       float s) {
  const float r = __fsub_rn(l, s);
  dh_add(my, dh_slot(x, p.lo[0], p.scale[0], bins));
  dh_add(my + S, dh_slot(l, p.lo[1], p.scale[1], bins));
  dh_add(my + 2 * S, dh_slot(s, p.lo[2], p.scale[2], bins));
  dh_add(my + 3 * S, dh_slot(r, p.lo[3], p.scale[3], bins));
}

// VEC: all three arrays are 16-byte aligned and the first n & ~3 rows go
// through float4 loads; otherwise every row takes the scalar loop.
template <bool VEC>
__global__ __launch_bounds__(DH_BLOCK) void drift_hist_kernel(
    const float* __restrict__ x, const float* __restrict__ l,
    const float* __restrict__ s, unsigned int* __restrict__ ws, long long n,
    int bins, DriftBins p) {
  __shared__ unsigned int h[DH_WAVES * DH_ROWS * (DH_MAX_BINS + 3)];
  const int S = bins + 3;
  const int W = DH_ROWS * S;
  for (int t = threadIdx.x; t < DH_WAVES * W; t += DH_BLOCK) h[t] = 0u;
  __syncthreads();
  unsigned int* my = h + (threadIdx.x >> 6) * W;

  const long long stride = (long long)gridDim.x * DH_BLOCK;
  const long long i = (long long)blockIdx.x * DH_BLOCK + threadIdx.x;
  const long long n4 = VEC ? (n & ~3ll) : 0ll;
  if (VEC) {
    for (long long j = i * 4; j < n4; j += stride * 4) {
      const float4 xv = *(const float4*)(x + j);
      const float4 lv = *(const float4*)(l + j);
      const float4 sv = *(const float4*)(s + j);
      dh_row(my, S, bins, p, xv.x, lv.x, sv.x);
      dh_row(my, S, bins, p, xv.y, lv.y, sv.y);
      dh_row(my, S, bins, p, xv.z, lv.z, sv.z);
      dh_row(my, S, bins, p, xv.w, lv.w, sv.w);
    }
  }
  for (long long j = n4 + i; j < n; j += stride)
    dh_row(my, S, bins, p, x[j], l[j], s[j]);

  __syncthreads();
  unsigned int* row = ws + (long long)blockIdx.x * W;
  for (int t = threadIdx.x; t < W; t += DH_BLOCK) {
    unsigned int c = 0u;
#pragma unroll
    for (int w = 0; w < DH_WAVES; ++w) c += h[w * W + t];
    row[t] = c;
  }
}
