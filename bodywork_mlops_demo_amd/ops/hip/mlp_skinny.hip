// Skinny-batch MLP scoring: the whole forward of 1..64 rows in ONE launch.
//
//   y[m] = b3 + sum_n w3[n] * relu(b2[n] + sum_k W2[n,k] * h1[m,k])
//   h1[m,k] = bf16(relu(xn[m] * w1[k] + b1[k])),  xn = (x - mu) / sigma
//
// At this shape the H x H weight matrix is all the traffic (32 MiB at
// H = 4096 against a few hundred activation bytes), so the kernel is built
// to stream W2 once, as wide as the chip is, and to keep everything else in
// registers:
//
//  * columns over workgroups: one workgroup (4 waves) owns 16 output columns
//    = one MFMA N-fragment; grid = H/16 (256 workgroups at H = 4096).
//  * K over the waves of a workgroup in 128-wide chunks, interleaved: wave w
//    takes chunks w, w+4, ...  A wave without a chunk (H < 512) adds zeros.
//  * B operand (weights): global memory -> registers, no LDS.  The order of
//    k inside an MFMA is free as long as A and B agree, so lane (fl, kg) owns
//    the 32 CONSECUTIVE k at k0 + kg*32 of row n0 + fl (four 16-byte loads of
//    one 64-byte run; the four lanes of a row cover 256 contiguous bytes) and
//    MFMA j of the chunk takes elements 8j..8j+7 of them.  Up to SK_AHEAD
//    chunks (the whole slab of a wave at H = 4096: 128 VGPRs) are requested
//    before the first MFMA.
//  * A operand (activations): never stored.  The lane evaluates layer 1 for
//    its row at the same permuted k with expand1d.h's arithmetic, so h1 is
//    the bits expand1d_bf16 writes, and it does so while the weights are in
//    flight.  xn is an IEEE subtract and divide.
//  * RF row fragments of 16 (1, 2 or 4) share the weight registers.
//  * epilogue: the four waves' accumulators are added through LDS in wave
//    order, then +b2, relu, *w3 and a butterfly over the 16 columns: one
//    fp32 partial per row and workgroup, written to a [grid, 16*RF] workspace.
//  * across workgroups, no float atomics: every workgroup fences (agent
//    scope) and draws a ticket with one integer atomic; the one that draws
//    the last fences again and adds the partials in a fixed order (16
//    segments of consecutive workgroups, each in index order, then the
//    segments in order), adds b3 and writes y.  No workgroup waits for
//    another, and the result is bitwise reproducible.
//
// n_dev (live_rows.h contract): rows at or past the count get an all-zero A
// fragment, their x is never read, and their y is exactly 0.  It saves no
// weight traffic: every workgroup streams its 16 rows of W2 regardless.
#include <ATen/cuda/CUDAContext.h>
#include <hip/hip_runtime.h>
#include <torch/extension.h>

#include "host_checks.h"
#include "live_rows.h"
#include "mfma_tile.h"
#include "mlp_fused.h"  // sk_a_frag, sk_combine, SK_* shared

constexpr int SK_COLS = 16;      // output columns of a workgroup
constexpr int SK_AHEAD = 8;      // chunks of a wave in flight (RF = 4: half)
constexpr int SK_MAX_M = 64;

// One workgroup per CU = one wave per SIMD: the wave may use the whole
// register file (the weight slab alone is 128 VGPRs), so the compiler is told
// not to trade registers for an occupancy the grid never reaches.
template <int RF>
__global__ __launch_bounds__(SK_THREADS)
__attribute__((amdgpu_waves_per_eu(1, 1))) void mlp_skinny_kernel(
    const float* __restrict__ x, float mu, float sigma,
    const bf16_t* __restrict__ w1, const bf16_t* __restrict__ b1,
    const bf16_t* __restrict__ W2, const float* __restrict__ b2,
    const float* __restrict__ w3, const float* __restrict__ b3,
    const int64_t* __restrict__ n_live, float* __restrict__ ws,
    unsigned int* __restrict__ ticket, float* __restrict__ y, int m, int H) {
  static_assert(RF == 1 || RF == 2 || RF == 4, "1, 2 or 4 row fragments");
  constexpr int ROWS = 16 * RF;
  // [wave][fragment*4 + reg][lane]; reused by the finalise
  __shared__ float red[SK_WAVES][RF * 4][64];
  __shared__ unsigned int drawn;

  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int fl = lane & 15;
  const int kg = lane >> 4;
  const int n0 = blockIdx.x * SK_COLS;
  const int live = n_live ? (int)live_count(n_live, m) : m;

  float xn[RF];
  bool alive[RF];
#pragma unroll
  for (int r = 0; r < RF; ++r) {
    const int row = r * 16 + fl;
    alive[r] = row < live;
    xn[r] = alive[r] ? (x[row] - mu) / sigma : 0.0f;
  }

  f32x4 acc[RF];
#pragma unroll
  for (int r = 0; r < RF; ++r) acc[r] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

  // One group = AHEAD chunks of every wave = GK consecutive k, in straight-
  // line phases: request the group's w1/b1 (two 16-byte loads per thread and
  // vector), request the weights, pass w1/b1 to the other waves through LDS,
  // evaluate layer 1 from LDS while the weights travel, multiply.  Vector
  // loads retire in issue order, so the w1/b1 requests go out first and the
  // wait for them leaves the weight loads in flight; the barrier orders LDS
  // only.  All waves run the same number of groups (the barriers are
  // uniform); a chunk past the end takes a valid address (chunk 0) and an
  // all-zero A fragment.
  constexpr int AHEAD = RF == 4 ? SK_AHEAD / 2 : SK_AHEAD;
  constexpr int GK = SK_WAVES * AHEAD * SK_CHUNK;
  constexpr int PIECES = GK / 8 / SK_THREADS;  // 16-byte pieces per thread
  __shared__ bf16_t s_w1[GK];
  __shared__ bf16_t s_b1[GK];
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
    bf16x8_v wv[AHEAD][4];
    unsigned int keep[AHEAD];
#pragma unroll
    for (int u = 0; u < AHEAD; ++u) {
      const int c = kb / SK_CHUNK + u * SK_WAVES + wave;
      keep[u] = c < nchunks ? ~0u : 0u;
      const int cc = c < nchunks ? c : 0;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        wv[u][j] = ((const lds_vec*)(wrow + cc * SK_CHUNK + j * 8))->v;
    }
    if (kb) {
      // A later group overwrites s_w1/s_b1: wait until every wave has read
      // the last group's.  A wave that arrives has issued its MFMAs, which
      // consumed every ds_read of that group; the clobbers keep the compiler
      // from moving an LDS access across the barrier (it is no memory
      // operation to it).
      asm volatile("" ::: "memory");
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
    bf16x8_v av[AHEAD][4][RF];
#pragma unroll
    for (int u = 0; u < AHEAD; ++u)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        // same k as wv[u][j], relative to the group
        const int c8 = (u * SK_WAVES + wave) * (SK_CHUNK / 8) + kg * 4 + j;
#pragma unroll
        for (int r = 0; r < RF; ++r)
          av[u][j][r] = sk_a_frag(xn[r], alive[r] ? keep[u] : 0u, s_w1, s_b1,
                                  c8);
      }
#pragma unroll
    for (int u = 0; u < AHEAD; ++u)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < RF; ++r)
          acc[r] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              av[u][j][r], wv[u][j], acc[r], 0, 0, 0);
  }

  // ---- the four K-slices of the workgroup, added in wave order -----------
#pragma unroll
  for (int r = 0; r < RF; ++r)
#pragma unroll
    for (int q = 0; q < 4; ++q) red[wave][r * 4 + q][lane] = acc[r][q];
  __syncthreads();
  // C layout: lane (fl, kg), reg q = row kg*4 + q of the fragment, column fl
  for (int r = wave; r < RF; r += SK_WAVES) {
    const float b2v = b2[n0 + fl];
    const float w3v = w3[n0 + fl];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float v = red[0][r * 4 + q][lane];
#pragma unroll
      for (int w = 1; w < SK_WAVES; ++w) v += red[w][r * 4 + q][lane];
      float t = fmaxf(v + b2v, 0.0f) * w3v;
#pragma unroll
      for (int s = 1; s < 16; s <<= 1) t += __shfl_xor(t, s, 64);
      if (fl == 0)
        ws[(long long)blockIdx.x * ROWS + r * 16 + kg * 4 + q] = t;
    }
  }

  // ---- ticket: the last workgroup to arrive adds up the partials ---------
  // red was last read above
  sk_combine<RF>(wave < RF, RF, &red[0][0][0], &drawn, ws, ticket, b3, y, m,
                 live);
}

// ---- host side --------------------------------------------------------------

at::Tensor mlp_skinny_score_hip(const at::Tensor& x, double mu, double sigma,
                                const at::Tensor& w1, const at::Tensor& b1,
                                const at::Tensor& w2, const at::Tensor& b2,
                                const at::Tensor& w3, const at::Tensor& b3,
                                const c10::optional<at::Tensor>& n_dev) {
  const char* op = "mlp_skinny_score";
  const MlpScoreOperands a = mlp_score_operands(op, SK_MAX_M, SK_CHUNK, x, w1,
                                                b1, w2, b2, w3, b3);
  const int64_t m = a.m, H = a.H;
  const int64_t* n_live = n_live_ptr(n_dev, x, op);

  const int rf = m <= 16 ? 1 : (m <= 32 ? 2 : 4);
  const int grid = (int)(H / SK_COLS);
  // fresh on every call (under capture: from the graph's pool, the zero
  // fill replayed with the graph), so there is no state to reset
  auto ws = at::empty({grid, 16 * rf}, x.options());
  auto ticket = at::zeros({1}, x.options().dtype(at::kInt));
  auto y = at::empty({m}, x.options());
  auto stream = at::cuda::getCurrentCUDAStream();
#define SK_LAUNCH(RF_)                                                       \
  hipLaunchKernelGGL((mlp_skinny_kernel<RF_>), dim3(grid), dim3(SK_THREADS), \
                     0, stream, x.data_ptr<float>(), (float)mu,              \
                     (float)sigma, (const bf16_t*)a.w1,                      \
                     (const bf16_t*)a.b1, (const bf16_t*)a.w2, a.b2, a.w3,   \
                     a.b3, n_live, ws.data_ptr<float>(),                     \
                     (unsigned int*)ticket.data_ptr<int>(),                  \
                     y.data_ptr<float>(), (int)m, (int)H)
  if (rf == 1) SK_LAUNCH(1);
  else if (rf == 2) SK_LAUNCH(2);
  else SK_LAUNCH(4);
#undef SK_LAUNCH
  return y;
}
