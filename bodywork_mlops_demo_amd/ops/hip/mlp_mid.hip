// Mini-batch MLP scoring: the whole forward of 1..256 rows in ONE launch,
// same arithmetic contract as mlp_skinny.hip:
//
//   y[m] = b3 + sum_n w3[n] * relu(b2[n] + sum_k W2[n,k] * h1[m,k])
//   h1[m,k] = bf16(relu(xn[m] * w1[k] + b1[k])),  xn = (x - mu) / sigma
//
// 256 rows are 16 MFMA row fragments.  The skinny kernel evaluates every
// layer-1 fragment of a K group ahead of its MFMAs and keeps them all in
// registers; at 16 fragments that is four register files.  By instruction
// count this kernel is bound by the layer-1 VALU work (every workgroup
// evaluates rows x H activations, ~24 VALU instructions per fragment against
// one MFMA), so the schedule is built around that:
//
//  * columns over workgroups, full K inside a workgroup: one workgroup
//    (4 waves) owns 16*CF = 32 output columns, grid = H / 32; relu and the w3
//    dot stay local, one fp32 partial per row crosses workgroups.
//  * K over the waves in 128-wide chunks, interleaved, and the B operand from
//    global memory straight into MFMA registers with the k permutation of the
//    skinny kernel (a lane owns 64 contiguous bytes of a row per chunk).  One
//    K group = 8/CF chunks of every wave (128 registers of weights, 2048 k),
//    all requested before the first MFMA; W2 is read once.
//  * the ROW FRAGMENTS are the rolled loop, four at a time: for a block of
//    four fragments the wave walks its weight registers once, evaluates the
//    A fragment of (row fragment, k step) with sk_a_frag just ahead of the
//    CF MFMAs that consume it, and keeps only 4*CF accumulators.  w1/b1 of a
//    k step are read from LDS and unpacked once per block of four.  The
//    accumulators of a finished block go to LDS ([wave][fragment]), which is
//    where the epilogue wants them anyway; with more than one K group they
//    are read back at the start of the next group's block.
//  * live count: blocks and fragments at or past the count are skipped by
//    wave-uniform branches (the count is a scalar), outside any barrier, so
//    layer-1 and MFMA work is proportional to ceil(n / 16); rows past the
//    count inside a live fragment get an all-zero A fragment, their x is
//    never read, and y is exactly 0 there.  The weight stream does not
//    depend on the count.
//  * epilogue: fragment r belongs to wave r % 4, which adds the four waves'
//    K slices in wave order, then +b2, relu, *w3, the CF column fragments in
//    order and a butterfly over 16 columns; ws is [grid, 256].  sk_combine
//    (mlp_fused.h) adds the workgroups' partials.
//
// Every row's sum has one fixed order (k inside a wave, waves, columns,
// workgroups), whatever m, the count or the other rows are: a live row's
// result is bitwise independent of them.
#include <ATen/cuda/CUDAContext.h>
#include <hip/hip_runtime.h>
#include <torch/extension.h>

#include "host_checks.h"
#include "live_rows.h"
#include "mfma_tile.h"
#include "mlp_fused.h"

constexpr int MID_MAX_M = 256;
constexpr int MID_FRAGS = MID_MAX_M / 16;
constexpr int MID_RB = 4;     // row fragments per pass over the weights
constexpr int MID_SLAB = 8;   // weight registers of a wave: 8 chunks x 16 rows
// CF, the column fragments of a workgroup.  Measured at H = 4096 (profiles/
// mid_scoring.md): 2 (32 columns, 128 workgroups, two K groups) was 3..8 us
// faster than 1 (16 columns, 256 workgroups, one K group) at every live
// count: an evaluated A fragment feeds two MFMAs.  Only 2 is built and
// tested; 4 does not fit this schedule (256 KB of accumulators in LDS).
constexpr int MID_CF = 2;

__global__ __launch_bounds__(SK_THREADS)
__attribute__((amdgpu_waves_per_eu(1, 1))) void mlp_mid_kernel(
    const float* __restrict__ x, float mu, float sigma,
    const bf16_t* __restrict__ w1, const bf16_t* __restrict__ b1,
    const bf16_t* __restrict__ W2, const float* __restrict__ b2,
    const float* __restrict__ w3, const float* __restrict__ b3,
    const int64_t* __restrict__ n_live, float* __restrict__ ws,
    unsigned int* __restrict__ ticket, float* __restrict__ y, int m, int H) {
  constexpr int CF = MID_CF;
  constexpr int AHEAD = MID_SLAB / CF;
  constexpr int GK = SK_WAVES * AHEAD * SK_CHUNK;
  constexpr int PIECES = GK / 8 / SK_THREADS;  // 16-byte pieces per thread
  // [wave][fragment][column fragment][reg][lane]; reused by the combine
  __shared__ float red[SK_WAVES][MID_FRAGS][CF][4][64];
  __shared__ bf16_t s_w1[GK];
  __shared__ bf16_t s_b1[GK];
  __shared__ float s_xn[MID_MAX_M];
  __shared__ unsigned int drawn;

  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int fl = lane & 15;
  const int kg = lane >> 4;
  const int n0 = blockIdx.x * (16 * CF);
  const int live = n_live ? (int)live_count(n_live, m) : m;
  const int nfrag = (live + 15) >> 4;

  // thread t standardises row t; the first barrier of the K loop publishes it
  s_xn[threadIdx.x] =
      (int)threadIdx.x < live ? (x[threadIdx.x] - mu) / sigma : 0.0f;

  // One group per pass of this loop, in the phases of the skinny kernel:
  // request w1/b1, request the weights, pass w1/b1 through LDS, then the row
  // fragment blocks.  All waves run the same number of groups (the barriers
  // are uniform); a chunk past the end takes a valid address (chunk 0) and an
  // all-zero A fragment.
  const int nchunks = H / SK_CHUNK;
  const bf16_t* wrow = W2 + (long long)(n0 + fl) * H + kg * 32;
  for (int kb = 0; kb < H; kb += GK) {
    bf16x8 w1g[PIECES], b1g[PIECES];
#pragma unroll
    for (int p = 0; p < PIECES; ++p) {
      const int k = kb + (p * SK_THREADS + (int)threadIdx.x) * 8;
      if (k < H) {
        w1g[p] = load_bf16x8(w1 + k);
        b1g[p] = load_bf16x8(b1 + k);
      }
    }
    bf16x8_v wv[AHEAD][4][CF];
    unsigned int keep[AHEAD];
#pragma unroll
    for (int u = 0; u < AHEAD; ++u) {
      const int c = kb / SK_CHUNK + u * SK_WAVES + wave;
      keep[u] = c < nchunks ? ~0u : 0u;
      const int cc = c < nchunks ? c : 0;
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int cf = 0; cf < CF; ++cf)
          wv[u][j][cf] = ((const lds_vec*)(wrow + (long long)cf * 16 * H +
                                           cc * SK_CHUNK + j * 8))->v;
    }
    if (kb) {
      // the last group's s_w1/s_b1 are overwritten: every wave has to be
      // through its blocks (the clobbers keep LDS accesses on their side of
      // the barrier, which is no memory operation to the compiler)
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
    }
#pragma unroll
    for (int p = 0; p < PIECES; ++p) {
      const int k = (p * SK_THREADS + (int)threadIdx.x) * 8;
      if (kb + k < H) {
        store_bf16x8(s_w1 + k, w1g[p]);
        store_bf16x8(s_b1 + k, b1g[p]);
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");

    // No barrier below: red[wave] is this wave's own until the epilogue.
#pragma unroll 1
    for (int f0 = 0; f0 < nfrag; f0 += MID_RB) {
      float xr[MID_RB];
      unsigned int kr[MID_RB];
      f32x4 acc[MID_RB][CF];
#pragma unroll
      for (int i = 0; i < MID_RB; ++i) {
        const int row = (f0 + i) * 16 + fl;
        xr[i] = s_xn[row];  // f0 <= 12, so row <= 255
        kr[i] = row < live ? ~0u : 0u;
#pragma unroll
        for (int cf = 0; cf < CF; ++cf) {
          acc[i][cf] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
          if (kb && f0 + i < nfrag) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
              acc[i][cf][q] = red[wave][f0 + i][cf][q][lane];
          }
        }
      }
#pragma unroll
      for (int u = 0; u < AHEAD; ++u)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          // same k as wv[u][j], relative to the group
          const int c8 = (u * SK_WAVES + wave) * (SK_CHUNK / 8) + kg * 4 + j;
#pragma unroll
          for (int i = 0; i < MID_RB; ++i) {
            // fragment f0 is live (f0 < nfrag); the others by a scalar test
            if (i == 0 || f0 + i < nfrag) {
              const bf16x8_v a =
                  sk_a_frag(xr[i], keep[u] & kr[i], s_w1, s_b1, c8);
#pragma unroll
              for (int cf = 0; cf < CF; ++cf)
                acc[i][cf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                    a, wv[u][j][cf], acc[i][cf], 0, 0, 0);
            }
          }
        }
#pragma unroll
      for (int i = 0; i < MID_RB; ++i)
        if (f0 + i < nfrag) {
#pragma unroll
          for (int cf = 0; cf < CF; ++cf)
#pragma unroll
            for (int q = 0; q < 4; ++q)
              red[wave][f0 + i][cf][q][lane] = acc[i][cf][q];
        }
    }
  }
  __syncthreads();

  // ---- the four K slices of a fragment, added in wave order ---------------
  // C layout: lane (fl, kg), reg q = row kg*4 + q of the fragment, column fl
  for (int r = wave; r < nfrag; r += SK_WAVES) {
    float t[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int cf = 0; cf < CF; ++cf) {
      const float b2v = b2[n0 + cf * 16 + fl];
      const float w3v = w3[n0 + cf * 16 + fl];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float v = red[0][r][cf][q][lane];
#pragma unroll
        for (int w = 1; w < SK_WAVES; ++w) v += red[w][r][cf][q][lane];
        const float h = fmaxf(v + b2v, 0.0f) * w3v;
        t[q] = cf ? t[q] + h : h;
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
      for (int s = 1; s < 16; s <<= 1) t[q] += __shfl_xor(t[q], s, 64);
      if (fl == 0)
        ws[(long long)blockIdx.x * MID_MAX_M + r * 16 + kg * 4 + q] = t[q];
    }
  }

  // red was last read above; the combine's first barrier is ahead of its
  // writes
  sk_combine<MID_FRAGS>(wave < nfrag, nfrag, &red[0][0][0][0][0], &drawn, ws,
                        ticket, b3, y, m, live);
}

// ---- host side --------------------------------------------------------------

at::Tensor mlp_mid_score_hip(const at::Tensor& x, double mu, double sigma,
                             const at::Tensor& w1, const at::Tensor& b1,
                             const at::Tensor& w2, const at::Tensor& b2,
                             const at::Tensor& w3, const at::Tensor& b3,
                             const c10::optional<at::Tensor>& n_dev) {
  const char* op = "mlp_mid_score";
  const MlpScoreOperands a = mlp_score_operands(op, MID_MAX_M, SK_CHUNK, x, w1,
                                                b1, w2, b2, w3, b3);
  const int64_t* n_live = n_live_ptr(n_dev, x, op);

  const int grid = (int)(a.H / (16 * MID_CF));
  // fresh on every call (under capture: from the graph's pool, the zero
  // fill replayed with the graph), so there is no state to reset
  auto ws = at::empty({grid, MID_MAX_M}, x.options());
  auto ticket = at::zeros({1}, x.options().dtype(at::kInt));
  auto y = at::empty({a.m}, x.options());
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(mlp_mid_kernel, dim3(grid), dim3(SK_THREADS), 0,
                     stream, x.data_ptr<float>(), (float)mu, (float)sigma,
                     (const bf16_t*)a.w1, (const bf16_t*)a.b1,
                     (const bf16_t*)a.w2, a.b2, a.w3, a.b3, n_live,
                     ws.data_ptr<float>(),
                     (unsigned int*)ticket.data_ptr<int>(),
                     y.data_ptr<float>(), (int)a.m, (int)a.H);
  return y;
}
