// What the one-kernel MLP scoring forwards (mlp_skinny.hip and its MXFP4
// twin mlp_skinny_mx4.hip: 1..64 rows, mlp_mid.hip and its MXFP4 twin
// mlp_mid_mx4.hip: 1..256 rows) share: the bf16 layer-1 MFMA A fragment, the
// quantised fp4 one, the skinny head, the combine of the
// workgroups' partial sums behind an integer ticket (their host entries share
// the checks of host_checks.h).  All of them run 4 waves, split K over them
// in 128-wide chunks and write one fp32 partial per row and workgroup.
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

// ---- the MXFP4 forwards (mlp_skinny_mx4.hip, mlp_mid_mx4.hip) ---------------
constexpr int SX_FMT = 4;  // the scaled MFMA's cbsz / blgp value for fp4

typedef __attribute__((ext_vector_type(8))) int sx_i32x8;
typedef __attribute__((ext_vector_type(4))) int sx_i32x4;

// the builtin takes 8 dwords whatever the format; fp4 reads the low four
__device__ __forceinline__ sx_i32x8 sx_operand(sx_i32x4 v) {
  return __builtin_shufflevector(v, v, 0, 1, 2, 3, -1, -1, -1, -1);
}

// Layer 1 of one row at the 32 columns 8*c8 .. 8*c8+31 (one MX block) as an
// fp4 MFMA A operand: codes and the block's E8M0 byte.  `keep` is all ones,
// or 0 for a dead row or a chunk past K: zero codes, byte 127 (an AND and a
// select, so that the w1/b1 reads and the quantiser stay outside any branch).
__device__ __forceinline__ sx_i32x4 sx_a_block(float xn, unsigned int keep,
                                               const bf16_t* __restrict__ w1,
                                               const bf16_t* __restrict__ b1,
                                               int c8, int& scale) {
  float h[4][8];
  unsigned int am = 0u;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    e1d_axpb<true, true>(xn, w1, b1, c8 + j, h[j]);
    am = max(am, mx4_amax8(h[j]));
  }
  const int e = mx4_block_exponent(am);
  sx_i32x4 q;
#pragma unroll
  for (int j = 0; j < 4; ++j) q[j] = (int)(mx4_pack8(h[j], e) & keep);
  scale = 127 + (e & (int)keep);
  return q;
}

// The skinny kernels' head: the four waves' accumulators of a workgroup's 16
// columns n0.. are added through LDS in wave order, then +b2, relu, *w3 and a
// butterfly over the 16 columns; one fp32 partial per row goes to
// ws[blockIdx.x][16*RF].  mlp_skinny_mx4.hip calls it; mlp_skinny.hip writes
// the same statements out in its kernel (built on this function its register
// allocation changes throughout, and that kernel is the measured baseline of
// profiles/skinny_scoring.md, so it is left as it was).  `red` is LDS for
// SK_WAVES * RF*4 * 64 floats, [wave][fragment*4 + reg][lane].  Call it with
// the whole block.  C layout: lane (fl, kg), reg q = row kg*4 + q of the
// fragment, column fl.
template <int RF, class Acc>
__device__ __forceinline__ void sk_head(const Acc (&acc)[RF], float* red,
                                        const float* __restrict__ b2,
                                        const float* __restrict__ w3,
                                        float* __restrict__ ws, int n0,
                                        int wave, int lane) {
  constexpr int ROWS = 16 * RF;
  const int fl = lane & 15;
  const int kg = lane >> 4;
#pragma unroll
  for (int r = 0; r < RF; ++r)
#pragma unroll
    for (int q = 0; q < 4; ++q)
      red[((wave * RF + r) * 4 + q) * 64 + lane] = acc[r][q];
  __syncthreads();
  for (int r = wave; r < RF; r += SK_WAVES) {
    const float b2v = b2[n0 + fl];
    const float w3v = w3[n0 + fl];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float v = red[(r * 4 + q) * 64 + lane];
#pragma unroll
      for (int w = 1; w < SK_WAVES; ++w)
        v += red[((w * RF + r) * 4 + q) * 64 + lane];
      float t = fmaxf(v + b2v, 0.0f) * w3v;
#pragma unroll
      for (int s = 1; s < 16; s <<= 1) t += __shfl_xor(t, s, 64);
      if (fl == 0)
        ws[(long long)blockIdx.x * ROWS + r * 16 + kg * 4 + q] = t;
    }
  }
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
