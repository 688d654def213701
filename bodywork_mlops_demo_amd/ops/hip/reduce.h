// Wave-64 / block reduction helpers for gfx950 (CDNA4: 64-lane waves).
#pragma once
#include <hip/hip_runtime.h>

// full-wave (64-lane) sum via xor shuffles
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__device__ __forceinline__ float wave_sum_f32(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__device__ __forceinline__ double wave_max_f64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
  return v;
}

// block-level sum: per-wave shuffle reduce -> LDS -> wave-0 combine.
// The combine order is fixed, so the result is bitwise reproducible.
// NWAVES = blockDim.x / 64 (<= 16).
template <int NWAVES>
__device__ __forceinline__ double block_sum_f64(double v, double* lds_scratch) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  v = wave_sum_f64(v);
  if (lane == 0) lds_scratch[wave] = v;
  __syncthreads();
  double total = 0.0;
  if (wave == 0) {
    total = (lane < NWAVES) ? lds_scratch[lane] : 0.0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) total += __shfl_xor(total, off, 64);
  }
  __syncthreads();  // scratch reusable by the caller afterwards
  return total;  // valid in wave 0 (all lanes)
}

// block-level max, same shape as block_sum_f64 (valid in wave 0).
template <int NWAVES>
__device__ __forceinline__ double block_max_f64(double v, double* lds_scratch) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  v = wave_max_f64(v);
  if (lane == 0) lds_scratch[wave] = v;
  __syncthreads();
  double total = 0.0;
  if (wave == 0) {
    total = lds_scratch[lane < NWAVES ? lane : 0];
    total = wave_max_f64(total);
  }
  __syncthreads();
  return total;
}
