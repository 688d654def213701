// Device side of the exact residual order statistic (resid_select.hip) —
// gfx950.  The k-th smallest |label - score| by a multi-pass radix select.
//
// THE KEY RULE.  For a row (label, score):
//   r   = fabsf(__fsub_rn(label, score))
//   key = __float_as_uint(r)
// For non-negative floats the unsigned key order is the value order, and
// bit 31 is 0.  A NaN residual (key > 0x7F800000) is excluded from the
// selection and counted; +inf (key == 0x7F800000) is an ordinary key, the
// largest.  ops/reference.py mirrors this in numpy float32.
//
// THE RANK.  With m the number of selected, non-NaN rows, level L asks for
// rank k = (int64)ceil((double)(m + 1) * L), two IEEE fp64 operations.
// k > m (m == 0 included) gives +inf, the conformal convention; otherwise
// the result is the k-th smallest key (1-based) reinterpreted as float.
//
// THE PASSES.  The 31 key bits are resolved in RS_PASSES = 3 digit passes of
// 11 + 10 + 10 bits, most significant first.  A pass
// (resid_select_pass_kernel) streams the two fp32 inputs once: float4 body +
// scalar tail, grid-stride, every row through the scalar loop when a view is
// not 16-byte aligned.  Pass 0 counts the top digit of every key into one
// table of 2048 bins, and NaN rows into slot 2048.  A later pass keeps one
// table of 1024 bins per level; a row is added to table q only when the
// bits above the pass's digit equal level q's prefix, which the prologue
// reads from the device state (so no host synchronisation between passes).
// Each wave adds into its own LDS copy with dh_add; after one barrier the
// block folds its waves' copies and writes them with plain stores into row
// blockIdx.x of a [grid, W] uint32 workspace, which drift_hist_finalize sums
// into int64.  No global atomics, no data-dependent loops; the counts are
// integers, so the result is exact, bitwise reproducible and independent of
// the grid.  Histograms of row shards add, which is what lets the caller
// all-reduce them between a pass and its pick.
//
// THE PICK (resid_select_pick_kernel, one block).  Per level: a block scan
// of the level's table finds the digit whose cumulative count reaches the
// remaining rank, appends it to the prefix and subtracts the count below it
// from the rank.  After pass 0 it first computes m, the NaN count and every
// k.
//
// THE STATE, int64[RS_STATE] in device memory:
//   [0] m   [1] NaN rows
//   [2 + 3q + 0] prefix of level q (the key bits resolved so far)
//   [2 + 3q + 1] remaining rank, 1-based within the rows that share the prefix
//   [2 + 3q + 2] 1 when k > m: the level is +inf and selects nothing
//
// LDS: 4 waves x tables x bins x 4 B, declared dynamically: 32.1 KB in pass 0,
// 16 / 32 / 48 / 64 KB in a later pass with 1 / 2 / 3 / 4 levels; 64 KB is
// the most a kernel may ask for without an opt-in attribute.
#pragma once
#include <hip/hip_runtime.h>

#include "lds_hist.h"
#include "philox.h"

#define RS_MAXQ 4
#define RS_PASSES 3
#define RS_BINS0 2048  // pass 0: key bits 30..20
#define RS_BINS 1024   // pass 1: bits 19..10, pass 2: bits 9..0
// pass-0 table: the bins, the NaN slot, padded to a multiple of 4
#define RS_W0 (RS_BINS0 + 4)
#define RS_NAN_SLOT RS_BINS0
#define RS_STATE (2 + 3 * RS_MAXQ)
#define RS_INF_KEY 0x7F800000u
// matches the high bits of no key: a level that selects nothing
#define RS_NO_PREFIX 0xFFFFFFFFu

// key bits below pass p's digit
__host__ __device__ __forceinline__ int rs_low_bits(int pass) {
  return pass == 0 ? 20 : pass == 1 ? 10 : 0;
}

struct ResidLevels {
  double L[RS_MAXQ];
};

// Where the rows come from.  Plain: (a, b) = (labels, scores), every row.
// SPLIT: (a, b) = (y, x), score = fmaf(coef, x, intercept) in fp32 exactly
// as linear_score_kernel computes it, and only the TEST rows of
// random_split count.
template <bool SPLIT>
struct ResidRows {
  const float* ab;  // SPLIT: device [intercept, coef]
  SplitKey key;
  float a, b;

  __device__ void begin() {
    if (SPLIT) { a = ab[0]; b = ab[1]; }
  }
  // the row's key; false when the row is not part of the source
  __device__ __forceinline__ bool row_key(long long i, float label, float p,
                                          unsigned int& k) const {
    if (SPLIT) p = fmaf(b, p, a);
    k = __float_as_uint(fabsf(__fsub_rn(label, p)));
    return SPLIT ? is_test_row(key, (unsigned long long)i) : true;
  }
};

// the prefixes of a later pass, uniform across the block
struct ResidPrefixes {
  unsigned int p[RS_MAXQ];
};

template <bool PASS0, bool SPLIT>
__device__ __forceinline__ void rs_row(unsigned int* my, int nq, int pass,
                                       const ResidPrefixes& pre,
                                       const ResidRows<SPLIT>& src,
                                       long long i, float a, float b) {
  unsigned int key;
  if (!src.row_key(i, a, b, key)) return;
  if (PASS0) {
    dh_add(my, key > RS_INF_KEY ? RS_NAN_SLOT : (int)(key >> 20));
  } else {
    if (key > RS_INF_KEY) return;
    const int low = rs_low_bits(pass);
    const unsigned int high = key >> (low + 10);
    const int digit = (int)((key >> low) & (RS_BINS - 1));
#pragma unroll
    for (int q = 0; q < RS_MAXQ; ++q)
      if (q < nq && high == pre.p[q]) dh_add(my + q * RS_BINS, digit);
  }
}

// W = RS_W0 (PASS0) or nq * RS_BINS; dynamic LDS = DH_WAVES * W * 4 bytes.
// VEC: both arrays are 16-byte aligned and the first n & ~3 rows go through
// float4 loads; otherwise every row takes the scalar loop.
template <bool PASS0, bool SPLIT, bool VEC>
__global__ __launch_bounds__(DH_BLOCK) void resid_select_pass_kernel(
    const float* __restrict__ a, const float* __restrict__ b,
    const long long* __restrict__ state, unsigned int* __restrict__ ws,
    long long n, int pass, int nq, ResidRows<SPLIT> src) {
  extern __shared__ unsigned int rs_lds[];
  const int W = PASS0 ? RS_W0 : nq * RS_BINS;
  for (int t = threadIdx.x; t < DH_WAVES * W; t += DH_BLOCK) rs_lds[t] = 0u;
  ResidPrefixes pre;
#pragma unroll
  for (int q = 0; q < RS_MAXQ; ++q) {
    pre.p[q] = RS_NO_PREFIX;
    if (!PASS0 && q < nq && state[2 + 3 * q + 2] == 0)
      pre.p[q] = (unsigned int)state[2 + 3 * q];
  }
  src.begin();
  __syncthreads();
  unsigned int* my = rs_lds + (threadIdx.x >> 6) * W;

  const long long stride = (long long)gridDim.x * DH_BLOCK;
  const long long i = (long long)blockIdx.x * DH_BLOCK + threadIdx.x;
  const long long n4 = VEC ? (n & ~3ll) : 0ll;
  if (VEC) {
    for (long long j = i * 4; j < n4; j += stride * 4) {
      const float4 av = *(const float4*)(a + j);
      const float4 bv = *(const float4*)(b + j);
      rs_row<PASS0, SPLIT>(my, nq, pass, pre, src, j, av.x, bv.x);
      rs_row<PASS0, SPLIT>(my, nq, pass, pre, src, j + 1, av.y, bv.y);
      rs_row<PASS0, SPLIT>(my, nq, pass, pre, src, j + 2, av.z, bv.z);
      rs_row<PASS0, SPLIT>(my, nq, pass, pre, src, j + 3, av.w, bv.w);
    }
  }
  for (long long j = n4 + i; j < n; j += stride)
    rs_row<PASS0, SPLIT>(my, nq, pass, pre, src, j, a[j], b[j]);

  __syncthreads();
  unsigned int* row = ws + (long long)blockIdx.x * W;
  for (int t = threadIdx.x; t < W; t += DH_BLOCK) {
    unsigned int c = 0u;
#pragma unroll
    for (int w = 0; w < DH_WAVES; ++w) c += rs_lds[w * W + t];
    row[t] = c;
  }
}

// One block.  hist is the int64 [RS_W0] (pass 0) or [nq, RS_BINS] table of
// the pass; out[q] is level q's key so far as a float (its unresolved low
// bits 0), the half-width itself after the last pass.
__global__ __launch_bounds__(DH_BLOCK) void resid_select_pick_kernel(
    const long long* __restrict__ hist, long long* __restrict__ state,
    float* __restrict__ out, int pass, int nq, ResidLevels lv) {
  __shared__ long long sc[DH_BLOCK];
  constexpr int CMAX = RS_BINS0 / DH_BLOCK;
  const int t = threadIdx.x;
  const int C = (pass == 0 ? RS_BINS0 : RS_BINS) / DH_BLOCK;  // bins a thread
  const int bits = pass == 0 ? 11 : 10;
  const int low = rs_low_bits(pass);
  for (int q = 0; q < nq; ++q) {
    const long long* tab = hist + (pass == 0 ? 0 : q * RS_BINS);
    // every thread reads the level's state before the barriers of the scan,
    // the one thread that finds the digit writes it after them
    long long prefix = 0, rank = 0, inf = 0;
    if (pass != 0) {
      prefix = state[2 + 3 * q];
      rank = state[2 + 3 * q + 1];
      inf = state[2 + 3 * q + 2];
    }
    long long c[CMAX];
    long long local = 0;
#pragma unroll
    for (int j = 0; j < CMAX; ++j) {
      c[j] = j < C ? tab[t * C + j] : 0;
      local += c[j];
    }
    // inclusive block scan of the per-thread counts
    sc[t] = local;
    __syncthreads();
#pragma unroll
    for (int off = 1; off < DH_BLOCK; off <<= 1) {
      const long long v = t >= off ? sc[t - off] : 0;
      __syncthreads();
      sc[t] += v;
      __syncthreads();
    }
    const long long incl = sc[t];
    const long long m = sc[DH_BLOCK - 1];
    __syncthreads();  // sc is written again for the next level
    if (pass == 0) {
      rank = (long long)ceil((double)(m + 1) * lv.L[q]);
      inf = rank > m;
      if (t == 0 && q == 0) {
        state[0] = m;
        state[1] = hist[RS_NAN_SLOT];
      }
    }
    if (inf) {
      if (t == 0) {
        state[2 + 3 * q] = 0;
        state[2 + 3 * q + 1] = 0;
        state[2 + 3 * q + 2] = 1;
        out[q] = __uint_as_float(RS_INF_KEY);
      }
    } else if (rank > incl - local && rank <= incl) {
      long long run = incl - local, below = run;
      int digit = 0;
      bool found = false;
#pragma unroll
      for (int j = 0; j < CMAX; ++j) {
        if (j < C && !found && rank <= run + c[j]) {
          digit = j;
          below = run;
          found = true;
        }
        run += c[j];
      }
      prefix = (prefix << bits) | (long long)(t * C + digit);
      state[2 + 3 * q] = prefix;
      state[2 + 3 * q + 1] = rank - below;
      state[2 + 3 * q + 2] = 0;
      out[q] = __uint_as_float((unsigned int)prefix << low);
    }
  }
}
