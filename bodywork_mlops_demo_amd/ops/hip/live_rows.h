// Device-side live row count: a captured scoring graph keeps its bucket-sized
// grid and reads the request's row count from device memory (int64[1]).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// the count, clamped to the buffer's [0, n] rows
__device__ __forceinline__ long long live_count(
    const int64_t* __restrict__ n_live, long long n) {
  long long live = (long long)*n_live;
  return live < 0 ? 0 : (live < n ? live : n);
}

// false: the row tile [m0, m0 + TILE_M) lies at or past the count and the
// caller returns; true: live_rows = its rows below the count, 1..TILE_M.
// Call it ahead of the first global_load_lds, barrier and LDS access: the
// test is block-uniform, so the whole block leaves together, and the count
// stays in SGPRs (the 16-wave kernels have no VGPR to spare).
template <int TILE_M>
__device__ __forceinline__ bool tile_live_rows(
    const int64_t* __restrict__ n_live, long long M, long long m0,
    int& live_rows) {
  const long long live = live_count(n_live, M);
  if (m0 >= live) return false;
  live_rows = (int)(live - m0 < TILE_M ? live - m0 : TILE_M);
  return true;
}
