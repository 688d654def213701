// Device side of the per-cell residual order statistic
// (resid_select_binned.hip) — gfx950.  Mondrian conformal: the k-th smallest
// |label - score| within each of up to 16 equal cells of x, every cell and
// every level resolved by the same streaming passes.
//
// THE CELL RULE.  Cells(n, lo, hi), 1 <= n <= 16, scale = fp32(n) /
// (fp32(hi) - fp32(lo)) computed once in Python and passed down.  For a
// row's x:
//   t = __fmul_rn(__fsub_rn(x, lo), scale)
//   cell = none   if t != t   (the row is left out, counted with the NaN rows)
//        = 0      else if t < 0
//        = n - 1  else if t >= n
//        = (int)t otherwise
// the slot rule of drift_hist.h without its under/overflow slots: x outside
// [lo, hi) clamps to an edge cell.  Single rounded fp32 operations, no FMA
// contraction; ops/reference.py mirrors it in numpy float32.
//
// KEY AND RANK are those of resid_select.h: key = float_as_uint(fabsf(
// __fsub_rn(label, score))), a NaN residual is left out and counted, +inf
// is the largest ordinary key, and level L of cell c asks for rank
// k = ceil((m_c + 1) * L) with the cell's own count m_c; k > m_c gives +inf.
//
// THE PASSES.  BS_PASSES = 4 digit passes of 8 + 8 + 8 + 7 key bits, most
// significant first, so that a table has 256 bins and 16 cells x 4 levels
// of them fit one block's LDS.  A pass (resid_select_binned_pass_kernel)
// streams x, labels, scores (12 B/row) or, split-linear, y and x (8 B/row,
// score and philox test flag evaluated in the kernel by ResidRows): float4
// body + scalar tail, grid-stride, all scalar when a view is not 16-byte
// aligned.  A block is BS_BLOCK = 1024 threads, 16 waves, and the grid is at
// most BS_GRID_CAP = 256 blocks (one per CU): a block's partial table is up
// to 64 KB, and fewer, larger blocks keep the [grid, W] workspace that
// carries the partials (and its finalise) small next to the 12 B/row
// stream.
//   pass 0   one table per cell, shared by the levels: slot c * 256 + (key
//            >> 23), and one slot (cells * 256) for every left-out row.
//            W = cells * 256 + 4.  Every row adds, and the top digit is the
//            exponent, so a few bins take most adds: BS_COPIES = 4 copies,
//            wave w adds into copy w & 3.
//   pass p>0 one table per (cell, level): a row of cell c is added to table
//            (c, q) when its key bits above the pass's digit equal that
//            pair's prefix.  W = cells * nq * 256.  The prefixes are read
//            from the device state into a [16][4] LDS array by the prologue
//            (no host synchronisation between passes) and a row fetches its
//            cell's four with one 16-byte LDS read.  Only the rows that
//            share a prefix add, spread over cells and digits: one table
//            shared by the block (four copies measured no faster on spread
//            or on constant rows, profiles/binned_conformal.md).
// Adds are dh_add (its uniform-slot shortcut serves constant data).  After
// one barrier the block folds its copies and writes row blockIdx.x of the
// [grid, W] uint32 workspace with plain stores; drift_hist_finalize sums the
// rows into int64.  No global atomics; exact integer counts, bitwise
// reproducible and independent of the grid.  Histograms of row shards add.
//
// LDS per block, declared dynamically (above 64 KB the launcher sets the
// opt-in attribute; the limit is 160 KB):
//   pass 0:  BS_COPIES * (cells * 256 + 4) * 4 B
//            1 cell 4.1 KB, 3 cells 12.1 KB, 16 cells 64.1 KB
//   pass p>0: cells * nq * 256 * 4 B (+ 256 B of prefixes, static)
//            16 cells: 16 / 32 / 48 / 64 KB with 1 / 2 / 3 / 4 levels
//
// THE PICK (resid_select_binned_pick_kernel): one block of 256 threads per
// cell, thread t owns bin t.  Per level a block scan of the table finds the
// digit whose cumulative count reaches the remaining rank, appends it to
// the prefix and subtracts the count below it from the rank.  After pass 0
// it first writes m_c and every rank, and block 0 the left-out count.
//
// THE STATE, int64 [cells, 2 + 3 * nq] in device memory, row c:
//   [0] m_c   [1] left-out (NaN) rows of the whole input, in row 0 only
//   [2 + 3q + 0] prefix of level q (the key bits resolved so far)
//   [2 + 3q + 1] remaining rank, 1-based within the rows sharing the prefix
//   [2 + 3q + 2] 1 when k > m_c: the level is +inf and selects nothing
//
// THE COVERAGE PASS (binned_coverage_kernel).  Per row one LDS add into slot
// cell * 16 + mask, mask bit q set when |label - score| <= h[cell][q]
// (plain <=, so an unused level passed as -1 never counts); a left-out row
// adds nothing.  The same two stages give int64 [cells * 16], and
// binned_coverage_fold_kernel turns them into [cells, 1 + 4]: the cell's
// rows, and per level the rows whose mask has the level's bit.
#pragma once
#include <hip/hip_runtime.h>

#include "lds_hist.h"
#include "philox.h"
// ResidRows, ResidLevels, RS_INF_KEY, RS_NO_PREFIX.  resid_select.h also
// defines its pick kernel, with external linkage; the unnamed namespace
// gives this translation unit a copy of its own (the headers above are
// already in, so only resid_select.h's own text lands inside).
namespace {
#include "resid_select.h"
}

#define BS_MAXC 16
#define BS_MAXQ RS_MAXQ
#define BS_PASSES 4
#define BS_BINS 256
#define BS_BLOCK 1024
#define BS_COPIES 4
#define BS_GRID_CAP 256
#define BS_MASKS 16  // 2^BS_MAXQ coverage masks per cell

// key bits below pass p's digit, and the digit's width
__host__ __device__ __forceinline__ int bs_low_bits(int pass) {
  return pass == 0 ? 23 : pass == 1 ? 15 : pass == 2 ? 7 : 0;
}
__host__ __device__ __forceinline__ int bs_digit_bits(int pass) {
  return pass == 3 ? 7 : 8;
}
__host__ __device__ __forceinline__ int bs_state_row(int nq) {
  return 2 + 3 * nq;
}

struct BinCells {
  int n;
  float lo, scale;
};

// the cell of x, -1 for none (NaN)
__device__ __forceinline__ int bs_cell(const BinCells& g, float x) {
  const float t = __fmul_rn(__fsub_rn(x, g.lo), g.scale);
  // the conversion is used only where 0 <= t < n
  int c = (int)t;
  c = t >= (float)g.n ? g.n - 1 : c;
  c = t < 0.f ? 0 : c;
  c = t != t ? -1 : c;
  return c;
}

// One row.  Plain: (x, a, b) = (x, label, score).  SPLIT: (x, a, b) = (x, y,
// x) and ResidRows scores x itself.
template <bool PASS0, bool SPLIT>
__device__ __forceinline__ void bs_row(unsigned int* tab,
                                       const uint4* __restrict__ pre, int nq,
                                       int pass, const BinCells& g,
                                       const ResidRows<SPLIT>& src,
                                       long long i, float x, float a,
                                       float b) {
  unsigned int key;
  if (!src.row_key(i, a, b, key)) return;
  const int c = bs_cell(g, x);
  const bool out = c < 0 || key > RS_INF_KEY;
  if (PASS0) {
    dh_add(tab, out ? g.n * BS_BINS : c * BS_BINS + (int)(key >> 23));
  } else {
    if (out) return;
    const int low = bs_low_bits(pass);
    const int bits = bs_digit_bits(pass);
    const unsigned int high = key >> (low + bits);
    const int digit = (int)((key >> low) & ((1u << bits) - 1u));
    const uint4 p = pre[c];
    // unused levels hold RS_NO_PREFIX, which no key's high bits equal
    const int slot = c * nq * BS_BINS + digit;
    if (high == p.x) dh_add(tab, slot);
    if (high == p.y) dh_add(tab, slot + BS_BINS);
    if (high == p.z) dh_add(tab, slot + 2 * BS_BINS);
    if (high == p.w) dh_add(tab, slot + 3 * BS_BINS);
  }
}

// W = cells * 256 + 4 (PASS0) or cells * nq * 256; dynamic LDS = copies * W
// * 4 bytes, copies = BS_COPIES (PASS0) or 1.  VEC: every array is 16-byte
// aligned and the first n & ~3 rows go through float4 loads.
template <bool PASS0, bool SPLIT, bool VEC>
__global__ __launch_bounds__(BS_BLOCK) void resid_select_binned_pass_kernel(
    const float* __restrict__ x, const float* __restrict__ a,
    const float* __restrict__ b, const long long* __restrict__ state,
    unsigned int* __restrict__ ws, long long n, int pass, int nq, int copies,
    BinCells g, ResidRows<SPLIT> src) {
  extern __shared__ unsigned int bs_lds[];
  __shared__ uint4 bs_pre[BS_MAXC];
  const int W = PASS0 ? g.n * BS_BINS + 4 : g.n * nq * BS_BINS;
  for (int t = threadIdx.x; t < copies * W; t += BS_BLOCK) bs_lds[t] = 0u;
  if (!PASS0 && threadIdx.x < BS_MAXC * BS_MAXQ) {
    const int c = threadIdx.x / BS_MAXQ, q = threadIdx.x % BS_MAXQ;
    unsigned int p = RS_NO_PREFIX;
    if (c < g.n && q < nq) {
      const long long* s = state + c * bs_state_row(nq) + 2 + 3 * q;
      if (s[2] == 0) p = (unsigned int)s[0];
    }
    ((unsigned int*)bs_pre)[threadIdx.x] = p;
  }
  src.begin();
  __syncthreads();
  unsigned int* tab = bs_lds + ((threadIdx.x >> 6) & (copies - 1)) * W;

  const long long stride = (long long)gridDim.x * BS_BLOCK;
  const long long i = (long long)blockIdx.x * BS_BLOCK + threadIdx.x;
  const long long n4 = VEC ? (n & ~3ll) : 0ll;
  if (VEC) {
    for (long long j = i * 4; j < n4; j += stride * 4) {
      const float4 xv = *(const float4*)(x + j);
      const float4 av = *(const float4*)(a + j);
      const float4 bv = SPLIT ? xv : *(const float4*)(b + j);
      bs_row<PASS0, SPLIT>(tab, bs_pre, nq, pass, g, src, j, xv.x, av.x, bv.x);
      bs_row<PASS0, SPLIT>(tab, bs_pre, nq, pass, g, src, j + 1, xv.y, av.y,
                           bv.y);
      bs_row<PASS0, SPLIT>(tab, bs_pre, nq, pass, g, src, j + 2, xv.z, av.z,
                           bv.z);
      bs_row<PASS0, SPLIT>(tab, bs_pre, nq, pass, g, src, j + 3, xv.w, av.w,
                           bv.w);
    }
  }
  for (long long j = n4 + i; j < n; j += stride) {
    const float xs = x[j];
    bs_row<PASS0, SPLIT>(tab, bs_pre, nq, pass, g, src, j, xs, a[j],
                         SPLIT ? xs : b[j]);
  }

  __syncthreads();
  unsigned int* row = ws + (long long)blockIdx.x * W;
  for (int t = threadIdx.x; t < W; t += BS_BLOCK) {
    unsigned int c = bs_lds[t];
    for (int w = 1; w < copies; ++w) c += bs_lds[w * W + t];
    row[t] = c;
  }
}

// grid = cells, BS_BINS threads.  hist is the int64 [cells * 256 + 4]
// (pass 0) or [cells, nq, 256] table of the pass; out[c, q] is the key so
// far as a float (its unresolved low bits 0), the half-width itself after
// the last pass.
__global__ __launch_bounds__(BS_BINS) void resid_select_binned_pick_kernel(
    const long long* __restrict__ hist, long long* __restrict__ state,
    float* __restrict__ out, int pass, int nq, ResidLevels lv) {
  __shared__ long long sc[BS_BINS];
  const int t = threadIdx.x;
  const int cell = blockIdx.x;
  const int bits = bs_digit_bits(pass);
  const int low = bs_low_bits(pass);
  long long* st = state + cell * bs_state_row(nq);
  for (int q = 0; q < nq; ++q) {
    const long long* tab =
        hist + (pass == 0 ? cell * BS_BINS : (cell * nq + q) * BS_BINS);
    // every thread reads the level's state before the barriers of the scan,
    // the one thread that finds the digit writes it after them
    long long prefix = 0, rank = 0, inf = 0;
    if (pass != 0) {
      prefix = st[2 + 3 * q];
      rank = st[2 + 3 * q + 1];
      inf = st[2 + 3 * q + 2];
    }
    const long long mine = tab[t];
    // inclusive block scan of the bins
    sc[t] = mine;
    __syncthreads();
#pragma unroll
    for (int off = 1; off < BS_BINS; off <<= 1) {
      const long long v = t >= off ? sc[t - off] : 0;
      __syncthreads();
      sc[t] += v;
      __syncthreads();
    }
    const long long incl = sc[t];
    const long long m = sc[BS_BINS - 1];
    __syncthreads();  // sc is written again for the next level
    if (pass == 0) {
      rank = (long long)ceil((double)(m + 1) * lv.L[q]);
      inf = rank > m;
      if (t == 0 && q == 0) {
        st[0] = m;
        st[1] = cell == 0 ? hist[gridDim.x * BS_BINS] : 0;
      }
    }
    if (inf) {
      if (t == 0) {
        st[2 + 3 * q] = 0;
        st[2 + 3 * q + 1] = 0;
        st[2 + 3 * q + 2] = 1;
        out[cell * nq + q] = __uint_as_float(RS_INF_KEY);
      }
    } else if (rank > incl - mine && rank <= incl) {
      prefix = (prefix << bits) | (long long)t;
      st[2 + 3 * q] = prefix;
      st[2 + 3 * q + 1] = rank - (incl - mine);
      st[2 + 3 * q + 2] = 0;
      out[cell * nq + q] = __uint_as_float((unsigned int)prefix << low);
    }
  }
}

// ---- coverage --------------------------------------------------------------
// W = cells * BS_MASKS; LDS BS_COPIES * W * 4 B (4 KB at 16 cells), static.
// h is fp32 [cells, 4] in device memory.
template <bool VEC>
__global__ __launch_bounds__(BS_BLOCK) void binned_coverage_kernel(
    const float* __restrict__ x, const float* __restrict__ s,
    const float* __restrict__ l, const float* __restrict__ h,
    unsigned int* __restrict__ ws, long long n, BinCells g) {
  __shared__ unsigned int cnt[BS_COPIES * BS_MAXC * BS_MASKS];
  __shared__ float4 hw[BS_MAXC];
  const int W = g.n * BS_MASKS;
  for (int t = threadIdx.x; t < BS_COPIES * W; t += BS_BLOCK) cnt[t] = 0u;
  if (threadIdx.x < g.n * BS_MAXQ) ((float*)hw)[threadIdx.x] = h[threadIdx.x];
  __syncthreads();
  unsigned int* tab = cnt + ((threadIdx.x >> 6) & (BS_COPIES - 1)) * W;

  auto row = [&](float xs, float sv, float lb) {
    const float r = fabsf(__fsub_rn(lb, sv));
    const int c = bs_cell(g, xs);
    if (c < 0 || r != r) return;
    const float4 hc = hw[c];
    const int mask = (r <= hc.x ? 1 : 0) | (r <= hc.y ? 2 : 0) |
                     (r <= hc.z ? 4 : 0) | (r <= hc.w ? 8 : 0);
    dh_add(tab, c * BS_MASKS + mask);
  };
  const long long stride = (long long)gridDim.x * BS_BLOCK;
  const long long i = (long long)blockIdx.x * BS_BLOCK + threadIdx.x;
  const long long n4 = VEC ? (n & ~3ll) : 0ll;
  if (VEC) {
    for (long long j = i * 4; j < n4; j += stride * 4) {
      const float4 xv = *(const float4*)(x + j);
      const float4 sv = *(const float4*)(s + j);
      const float4 lb = *(const float4*)(l + j);
      row(xv.x, sv.x, lb.x);
      row(xv.y, sv.y, lb.y);
      row(xv.z, sv.z, lb.z);
      row(xv.w, sv.w, lb.w);
    }
  }
  for (long long j = n4 + i; j < n; j += stride) row(x[j], s[j], l[j]);

  __syncthreads();
  for (int t = threadIdx.x; t < W; t += BS_BLOCK) {
    unsigned int c = 0u;
#pragma unroll
    for (int w = 0; w < BS_COPIES; ++w) c += cnt[w * W + t];
    ws[(long long)blockIdx.x * W + t] = c;
  }
}

// one thread per output: out[c, 0] = rows of cell c, out[c, 1 + q] = those
// whose mask has bit q
__global__ void binned_coverage_fold_kernel(
    const long long* __restrict__ masks, long long* __restrict__ out,
    int cells) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= cells * (1 + BS_MAXQ)) return;
  const int c = t / (1 + BS_MAXQ), j = t % (1 + BS_MAXQ);
  long long sum = 0;
  for (int k = 0; k < BS_MASKS; ++k)
    if (j == 0 || ((k >> (j - 1)) & 1)) sum += masks[c * BS_MASKS + k];
  out[t] = sum;
}
