// What the LDS histogram kernels share (drift_hist.h, resid_select.h) —
// gfx950: the block shape, the wave-aggregated LDS add and the finalise
// that sums a [grid, W] uint32 workspace into int64.
#pragma once
#include <hip/hip_runtime.h>

#define DH_BLOCK 256
#define DH_WAVES (DH_BLOCK / 64)
// stage 2: DH_FIN_SLOTS slots per block in quads, DH_FIN_PARTS threads per
// quad
#define DH_FIN_SLOTS 32
#define DH_FIN_PARTS (DH_BLOCK / (DH_FIN_SLOTS / 4))

// tab[slot] += 1 for every active lane.  Results unused: no-return
// ds_add_u32.  When all active lanes of the wave hold the same slot (a
// constant column, a column of NaN) one lane adds their count, which keeps
// 64 same-address adds from serialising; measured no slower on spread data
// (profiles/drift_histograms.md).
__device__ __forceinline__ void dh_add(unsigned int* tab, int slot) {
  const int first = __builtin_amdgcn_readfirstlane(slot);
  const unsigned long long act = __ballot(1);
  if (__ballot(slot == first) == act) {
    if ((int)__lane_id() == (int)__builtin_ctzll(act))
      __hip_atomic_fetch_add(tab + first, (unsigned int)__popcll(act),
                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  } else {
    __hip_atomic_fetch_add(tab + slot, 1u, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_WORKGROUP);
  }
}

// out[t] = sum over g < nblocks of ws[g, t], t < W (W is a multiple of 4).
// Block b owns slots [b * DH_FIN_SLOTS, (b + 1) * DH_FIN_SLOTS); thread
// (part, quad) sums four consecutive slots of workspace rows part, part +
// DH_FIN_PARTS, ... with 16-byte loads, consecutive threads on consecutive
// quads, and the parts meet in LDS.  static: every translation unit that
// includes this header gets its own copy.
static __global__ __launch_bounds__(DH_BLOCK) void drift_hist_finalize(
    const unsigned int* __restrict__ ws, long long* __restrict__ out,
    int nblocks, int W) {
  __shared__ long long part[DH_FIN_PARTS][DH_FIN_SLOTS];
  constexpr int QUADS = DH_FIN_SLOTS / 4;
  const int q = threadIdx.x % QUADS;
  const int pt = threadIdx.x / QUADS;
  const int t = blockIdx.x * DH_FIN_SLOTS + q * 4;
  long long acc[4] = {0, 0, 0, 0};
  if (t < W) {
    for (int g = pt; g < nblocks; g += DH_FIN_PARTS) {
      const uint4 c = *(const uint4*)(ws + (long long)g * W + t);
      acc[0] += c.x;
      acc[1] += c.y;
      acc[2] += c.z;
      acc[3] += c.w;
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) part[pt][q * 4 + k] = acc[k];
  __syncthreads();
  const int o = blockIdx.x * DH_FIN_SLOTS + threadIdx.x;
  if (threadIdx.x < DH_FIN_SLOTS && o < W) {
    long long sum = 0;
#pragma unroll
    for (int p = 0; p < DH_FIN_PARTS; ++p) sum += part[p][threadIdx.x];
    out[o] = sum;
  }
}
