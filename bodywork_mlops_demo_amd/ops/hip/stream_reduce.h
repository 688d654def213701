// Stage 1 of every streaming fp64 reduction over two fp32 inputs — gfx950.
//
// One kernel, stream_reduce2_kernel<Stat>, owns the float4 body, the scalar
// tail, the four lane accumulators, their fold and the per-block reduction
// into a [grid, K] workspace row; a statistic type says only WHAT is summed.
// A new fused statistic is a new Stat type, never a new loop.
//
// A Stat declares
//   static constexpr int  NSUM     how many sums it keeps
//   static constexpr int  MAX_POS  where its one max sits among the sums in
//                                  the workspace row (-1: it has none)
//   static constexpr bool COUNTS   whether the row starts with a row count
//   __device__ void begin()        once per thread, ahead of the first row:
//                                  fetch what row() needs from memory
//   __device__ void row(i, a, b, sum, mx, cnt) const
//                                  fold row i = (a[i], b[i]) into the sums
//                                  (sum[k] in workspace order), the max and
//                                  the per-thread count (rows < 2^32)
// and the workspace row is [cnt?] + the sums in order with the max inserted
// at MAX_POS.  K, the finalise kernel's max_mask and its output offset are
// derived from these (stat_layout<Stat>), never passed as literals.
#pragma once
#include <hip/hip_runtime.h>

#include "reduce.h"

#define RED_BLOCK 256
#define RED_WAVES (RED_BLOCK / 64)

template <class Stat>
struct stat_layout {
  static constexpr bool HAS_MAX = Stat::MAX_POS >= 0;
  // statistics per workspace row
  static constexpr int K = (Stat::COUNTS ? 1 : 0) + Stat::NSUM + (HAS_MAX ? 1 : 0);
  // bit k set: statistic k of the row is a max, else a sum
  static constexpr unsigned int MAX_MASK =
      HAS_MAX ? 1u << ((Stat::COUNTS ? 1 : 0) + Stat::MAX_POS) : 0u;
  // the result is [n] + row without a count of its own, else the row
  static constexpr int OFF = Stat::COUNTS ? 0 : 1;
};

// per-wave shuffle -> LDS -> one plain store by thread 0: the block's value
// of one statistic goes to ws[idx]
template <bool IS_MAX>
__device__ __forceinline__ void block_reduce_store(double v, double* lds,
                                                   double* ws, long long idx) {
  const double t = IS_MAX ? block_max_f64<RED_WAVES>(v, lds)
                          : block_sum_f64<RED_WAVES>(v, lds);
  if (threadIdx.x == 0) ws[idx] = t;
}

template <class Stat>
__global__ void stream_reduce2_kernel(const float* __restrict__ a,
                                      const float* __restrict__ b,
                                      double* __restrict__ ws, long long n,
                                      Stat s) {
  using L = stat_layout<Stat>;
  constexpr int NSUM = Stat::NSUM;
  // 4 independent partial accumulators per sum (one per float4 lane) break
  // the per-iteration fp64 dependency chains that left the serial version
  // at ~12% of HBM bandwidth
  double sum[4][NSUM] = {};
  double mx = 0;
  unsigned int cnt = 0;
  s.begin();
  const long long stride = (long long)gridDim.x * RED_BLOCK;
  const long long i = (long long)blockIdx.x * RED_BLOCK + threadIdx.x;
  const long long n4 = n & ~3ll;
  for (long long j = i * 4; j < n4; j += stride * 4) {
    float4 av = *(const float4*)(a + j);
    float4 bv = *(const float4*)(b + j);
    const float as[4] = {av.x, av.y, av.z, av.w};
    const float bs[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) s.row(j + e, as[e], bs[e], sum[e], mx, cnt);
  }
  for (long long j = n4 + i; j < n; j += stride)
    s.row(j, a[j], b[j], sum[0], mx, cnt);
#pragma unroll
  for (int e = 1; e < 4; ++e) {
#pragma unroll
    for (int k = 0; k < NSUM; ++k) sum[0][k] += sum[e][k];
  }
  double* row = ws + (long long)blockIdx.x * L::K;
  __shared__ double lds[RED_WAVES];
  if (Stat::COUNTS) block_reduce_store<false>((double)cnt, lds, row++, 0);
#pragma unroll
  for (int k = 0; k < NSUM + (L::HAS_MAX ? 1 : 0); ++k) {
    if (k == Stat::MAX_POS)
      block_reduce_store<true>(mx, lds, row, k);
    else
      block_reduce_store<false>(
          sum[0][k - (L::HAS_MAX && k > Stat::MAX_POS ? 1 : 0)], lds, row, k);
  }
}
