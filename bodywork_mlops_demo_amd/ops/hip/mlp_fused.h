// What the one-kernel MLP scoring forwards (mlp_skinny.hip: 1..64 rows,
// mlp_mid.hip: 1..256 rows) share: the layer-1 MFMA A fragment, the combine
// of the workgroups' partial sums behind an integer ticket (their host
// entries share mlp_score_operands, host_checks.h).  Both kernels run 4
// waves, split K over them in 128-wide chunks and write one fp32 partial per
// row and workgroup.
#pragma once
#include <hip/hip_runtime.h>

#include "bf16_utils.h"
#include "expand1d.h"

constexpr int SK_THREADS = 256;  // 4 waves
constexpr int SK_WAVES = 4;
constexpr int SK_CHUNK = 128;    // k of one wave step = 4 MFMAs of K=32
constexpr int SK_SEGS = 16;      // combine: segments of consecutive blocks

// layer 1 of one row at columns 8*c8 .. 8*c8+7 as an MFMA A fragment; `keep`
// is all ones, or 0 for a dead row (an AND, so that the loads stay outside
// any branch)
__device__ __forceinline__ bf16x8_v sk_a_frag(float xn, unsigned int keep,
                                              const bf16_t* __restrict__ w1,
                                              const bf16_t* __restrict__ b1,
                                              int c8) {
  float h[8];
  e1d_axpb<true, true>(xn, w1, b1, c8, h);
  const bf16x8 packed = f32_to_bf16x8(h);
  union {
    bf16x8_v v;
    unsigned int u[4];
  } f;
  __builtin_memcpy(&f, &packed, sizeof(f));
#pragma unroll
  for (int e = 0; e < 4; ++e) f.u[e] &= keep;
  return f.v;
}

// The last workgroup to arrive adds up the partials ws[grid][16*RF] of row
// fragments 0..nfrag-1 and writes y; call it with the whole block, last thing
// in the kernel.  `wrote`: this wave stored partials.  `part` is LDS for
// RF*SK_SEGS*16 floats that nobody reads any more, `drawn` one LDS word.
// Agent-scope fences (the XCDs' L2s are not coherent for plain accesses):
// each wave that wrote partials releases them, thread 0 releases again
// behind the barrier and draws; the last workgroup acquires before it
// reads.  Waves that wrote nothing do not fence: a fence is an L2
// writeback and invalidate, and 1024 waves would queue them.  No float
// atomics and a fixed order (SK_SEGS segments of consecutive workgroups,
// each in index order, then the segments in order): bitwise reproducible.
template <int RF>
__device__ __forceinline__ void sk_combine(
    bool wrote, int nfrag, float* part, unsigned int* drawn,
    const float* __restrict__ ws, unsigned int* __restrict__ ticket,
    const float* __restrict__ b3, float* __restrict__ y, int m, int live) {
  constexpr int ROWS = 16 * RF;
  if (wrote) __threadfence();
  __syncthreads();
  if (threadIdx.x == 0) {
    __threadfence();
    *drawn = atomicAdd(ticket, 1u);
  }
  __syncthreads();
  if (*drawn != gridDim.x - 1) return;
  __threadfence();

  const int grid = (int)gridDim.x;
  const int per = (grid + SK_SEGS - 1) / SK_SEGS;
  {
    const int seg = threadIdx.x >> 4;
    const int r16 = threadIdx.x & 15;
    const int g0 = seg * per;
    const int g1 = min(g0 + per, grid);
#pragma unroll
    for (int r = 0; r < RF; ++r) {
      if (r >= nfrag) break;
      float s = 0.0f;
#pragma unroll 8
      for (int g = g0; g < g1; ++g)
        s += __hip_atomic_load(ws + (long long)g * ROWS + r * 16 + r16,
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      part[(r * SK_SEGS + seg) * 16 + r16] = s;
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < ROWS && (int)threadIdx.x < m) {
    const int row = threadIdx.x;
    const int r = row >> 4, r16 = row & 15;
    float s = 0.0f;
    if (row < live) {
#pragma unroll
      for (int seg = 0; seg < SK_SEGS; ++seg)
        s += part[(r * SK_SEGS + seg) * 16 + r16];
      s += b3[0];
    }
    y[row] = s;
  }
}
