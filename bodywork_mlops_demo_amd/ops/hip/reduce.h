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

// ---- many sums per lane: halving butterfly ---------------------------------
// wave_sum_f64 on each of K per-lane values costs 6 K shuffles.  Here the
// lanes split the statistics while they sum them: at offset 32, 16, .., 1 a
// lane whose bit is clear keeps the lower half of its values, its partner
// the upper half, and each adds the other's copy of the half it keeps.  The
// value count halves per step (K + K/2 + .. ~ K shuffles in all), and every
// statistic goes through the pairing tree of the xor butterfly, so its sum
// has the bits wave_sum_f64 gives.  Afterwards v[e], e <
// wave_scatter_len<K>(), is the wave's sum of statistic
// wave_scatter_index<K>(e, lane) (-1: a padding slot).
__host__ __device__ constexpr int wave_scatter_half(int k, int steps) {
  return steps == 0 ? k : wave_scatter_half((k + 1) / 2, steps - 1);
}

template <int K>
__host__ __device__ constexpr int wave_scatter_len() {
  return wave_scatter_half(K, 6);
}

template <int KS, int OFF, int N>
__device__ __forceinline__ void wave_scatter_step(double (&v)[N], bool upper) {
  constexpr int H = (KS + 1) / 2;
#pragma unroll
  for (int k = 0; k < H; ++k) {
    const double lo = v[k];
    const double hi = (k + H < KS) ? v[k + H] : 0.0;
    const double keep = upper ? hi : lo;
    const double send = upper ? lo : hi;
    v[k] = keep + __shfl_xor(send, OFF, 64);
  }
}

template <int K>
__device__ __forceinline__ void wave_sum_scatter_f64(double (&v)[K], int lane) {
  wave_scatter_step<wave_scatter_half(K, 0), 32>(v, lane & 32);
  wave_scatter_step<wave_scatter_half(K, 1), 16>(v, lane & 16);
  wave_scatter_step<wave_scatter_half(K, 2), 8>(v, lane & 8);
  wave_scatter_step<wave_scatter_half(K, 3), 4>(v, lane & 4);
  wave_scatter_step<wave_scatter_half(K, 4), 2>(v, lane & 2);
  wave_scatter_step<wave_scatter_half(K, 5), 1>(v, lane & 1);
}

// which statistic slot e of this lane holds: undo the six splits, last first
template <int K>
__device__ __forceinline__ int wave_scatter_index(int e, int lane) {
  int idx = e;
  bool live = true;
#pragma unroll
  for (int s = 5; s >= 0; --s) {
    if (lane & (32 >> s)) idx += wave_scatter_half(K, s + 1);
    live = live && idx < wave_scatter_half(K, s);
  }
  return live ? idx : -1;
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
