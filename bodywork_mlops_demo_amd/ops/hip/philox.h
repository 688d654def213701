// philox4x32-10 counter-based RNG — device-side, gfx950.
//
// Bit-identical to the numpy implementation in ops/reference.py
// (the CPU oracle): counter i expands to the 128-bit counter
// (lo32(i), hi32(i), 0, 0); key = (seed_lo, seed_hi or 0x1F123BB5).
// Replaces the reference's numpy RNG draws (stage_3:39-40) on-GPU.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#define PHILOX_M0 0xD2511F53u
#define PHILOX_M1 0xCD9E8D57u
#define PHILOX_W0 0x9E3779B9u
#define PHILOX_W1 0xBB67AE85u

struct Philox4 {
  unsigned int x, y, z, w;
};

__device__ __forceinline__ Philox4 philox4x32(unsigned long long counter,
                                              unsigned int key0,
                                              unsigned int key1) {
  unsigned int c0 = (unsigned int)(counter & 0xFFFFFFFFull);
  unsigned int c1 = (unsigned int)(counter >> 32);
  unsigned int c2 = 0u, c3 = 0u;
  unsigned int k0 = key0, k1 = key1;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    unsigned long long p0 = (unsigned long long)PHILOX_M0 * c0;
    unsigned long long p1 = (unsigned long long)PHILOX_M1 * c2;
    unsigned int hi0 = (unsigned int)(p0 >> 32), lo0 = (unsigned int)p0;
    unsigned int hi1 = (unsigned int)(p1 >> 32), lo1 = (unsigned int)p1;
    unsigned int n0 = hi1 ^ c1 ^ k0;
    unsigned int n1 = lo1;
    unsigned int n2 = hi0 ^ c3 ^ k1;
    unsigned int n3 = lo0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += PHILOX_W0;
    k1 += PHILOX_W1;
  }
  return {c0, c1, c2, c3};
}

// ---- the project's philox streams, side by side ---------------------------
// key = (lo32(seed), hi32(seed)); a seed that fits 32 bits takes the
// stream's own default second key word instead, so the data generator, the
// train/test split and the cross-validation folds never draw from the same
// stream for one seed (ops/reference.py: datagen_cpu / _SPLIT_KEY1 /
// _FOLD_KEY1).
#define PHILOX_DATAGEN_KEY1 0x1F123BB5u
#define PHILOX_SPLIT_KEY1 0x85EBCA6Bu

struct PhiloxKey {
  unsigned int key0, key1;
};

static inline PhiloxKey philox_key(int64_t seed, unsigned int default_key1) {
  return {(unsigned int)(seed & 0xFFFFFFFFll),
          (seed > 0xFFFFFFFFll) ? (unsigned int)(seed >> 32) : default_key1};
}

static inline PhiloxKey datagen_key(int64_t seed) {
  return philox_key(seed, PHILOX_DATAGEN_KEY1);
}

// The train/test split: row i is a TEST row iff philox(key, i).x < tau,
// tau = test_frac * 2^32.  random_split and the fused linear fit
// (linreg_split_stats / linear_split_metrics) all ask is_test_row, so they
// see the same row sets by construction.
struct SplitKey {
  unsigned int key0, key1, tau;
};

static inline SplitKey split_key(int64_t seed, double test_frac) {
  const PhiloxKey k = philox_key(seed, PHILOX_SPLIT_KEY1);
  return {k.key0, k.key1, (unsigned int)(test_frac * 4294967296.0)};
}

__device__ __forceinline__ bool is_test_row(const SplitKey& k,
                                            unsigned long long i) {
  return philox4x32(i, k.key0, k.key1).x < k.tau;
}

// The cross-validation folds, a third stream: row i belongs to fold
// (philox(key, i).x * folds) >> 32, in [0, folds)
// (ops/reference.py: fold_ids_cpu / _FOLD_KEY1).
#define PHILOX_FOLD_KEY1 0xC2B2AE35u

static inline PhiloxKey fold_key(int64_t seed) {
  return philox_key(seed, PHILOX_FOLD_KEY1);
}

__device__ __forceinline__ unsigned int fold_of_row(const PhiloxKey& k,
                                                    unsigned long long i,
                                                    unsigned int folds) {
  return (unsigned int)(((unsigned long long)philox4x32(i, k.key0, k.key1).x *
                         folds) >> 32);
}

// uniform in [0,1): u32 * 2^-32 (matches the numpy oracle's float32 math)
__device__ __forceinline__ float u32_to_uniform(unsigned int r) {
  return (float)r * 2.3283064365386963e-10f;  // 1/2^32
}
