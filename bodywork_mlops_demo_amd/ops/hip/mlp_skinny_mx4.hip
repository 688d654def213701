// Skinny-batch MLP scoring on MXFP4 weights: the whole forward of 1..64 rows
// in ONE launch, streaming the model's 4-bit shadow of W2 instead of bf16.
//
//   y[m] = b3 + sum_n w3[n] * relu(b2[n] + sum_k dq(W2)[n,k] * dq(h1)[m,k])
//   h1[m,k] = relu(xn[m] * w1[k] + b1[k]) in fp32,  xn = (x - mu) / sigma
//
// dq(.) is the MXFP4 decode (e2m1 code times the E8M0 scale of its 32-block).
// W2 arrives quantised (ops.quantize_mxfp4: codes [H, H/2], scales in
// mx4_scale_index order, expand1d.h); h1 is quantised here, in registers, to
// the bits ops.expand1d_mxfp4 writes.  The matrix instruction is the fp4 form
// (cbsz = blgp = 4) of v_mfma_scale_f32_16x16x128_f8f6f4.  At this shape the
// weights are all the traffic: 8.5 MiB at H = 4096 against 32 MiB of bf16.
//
// Layout.  The skeleton is mlp_skinny.hip's:
//
//  * one workgroup (4 waves) owns 16 output columns n0..n0+15; grid = H/16.
//  * K over the waves in 128-wide chunks, interleaved: wave w takes chunks w,
//    w+4, ...  One chunk is ONE K=128 MFMA per row fragment.  A wave without
//    a chunk (H < 512) adds zeros.
//  * a K group is SX_AHEAD = 8 chunks of every wave = 4096 k, for every RF; a
//    larger H runs the group loop again.
//  * B operand (weight codes): global memory -> operand registers, no LDS.
//    Lane (fl, kg) of chunk c supplies one whole 32-block, block 4c+kg of row
//    n0+fl: ONE 16-byte load.  The four kg lanes of a row cover 64
//    contiguous bytes, so a load instruction of the wave reads 16 half
//    cache lines whole.  The slab of a wave at H = 4096 is 8 chunks x 4 = 32
//    VGPRs, all requested before the first MFMA.
//  * B scales: block 4c+kg of row n0+fl sits at byte
//      ((G*nt + (c>>1))*64 + kg*16 + fl)*8 + (c&1)*4 + i,
//    G = n0>>6, i = (n0>>4)&3, nt = H/256 (mx4_scale_index with the row and
//    block above).  c&1 = wave&1 for every chunk of a wave, so the lane
//    loads the ONE dword (c&1) that holds its byte: 8 dword loads per group,
//    requested with the codes.  i is workgroup-uniform but no compile-time
//    constant, so the byte is shifted to position 0 and the MFMA's op_sel
//    stays 0.
//  * A operand (activations): never stored.  Lane (fl, kg) evaluates layer 1
//    for row 16r+fl at the 32 k of block 4c+kg from the LDS copy of w1/b1
//    (e1d_axpb<true, true>: fp32 fmaf, relu, no bf16 rounding), takes the
//    block amax over its OWN 32 values (the lane's operand is exactly one MX
//    block: no cross-lane step), and quantises with the quantiser's own
//    arithmetic (mx4_amax8 / mx4_block_exponent / mx4_pack8, expand1d.h): 4
//    VGPRs of codes and the scale byte e + 127, which the same lane hands to
//    the MFMA.  A dead row, or a chunk past the end of K, supplies all-zero
//    codes with scale byte 127 (2^0); byte 255 (NaN) is never generated (e
//    is clamped to [-127, 127]).
//  * RF row fragments of 16 (1, 2 or 4) share the weight registers.
//  * epilogue and combine: sk_head and sk_combine (mlp_fused.h), the bf16
//    skinny kernel's arithmetic in the same order: bitwise reproducible.
//
// Landing of the loads.  Everything is plain C++, so the compiler counts
// vmcnt; vector memory loads retire in issue order.  Per group a wave issues,
// in program order, its w1/b1 pieces (up to 4 loads), then the 8 chunks'
// codes (dwordx4) and scale dwords: 16 more, all ahead of the first barrier.
// The waits ahead of the LDS stores cover the w1/b1 loads only (vmcnt(17),
// vmcnt(16) in the built code) and leave the 16 weight loads in flight
// through the barrier and the whole of layer 1; the MFMAs then count down
// from vmcnt(15)/vmcnt(14) ahead of the first to vmcnt(0) ahead of the last,
// each waiting for its own codes and scale.  The counts are the compiler's,
// so a different schedule can only move them, never leave a register read
// uncovered.  No load is in flight at the epilogue.
//
// Barriers and LDS reuse in the group loop.  s_w1/s_b1 are written once per
// group.  Group g > 0 overwrites them, so every wave first passes a barrier
// that it reaches only after its layer-1 phase of group g-1 (all its ds_reads
// of s_w1/s_b1 feed the quantiser whose results the MFMAs above the barrier
// consumed); then the stores, s_waitcnt lgkmcnt(0), a second barrier, and
// the reads.  All waves run the same number of groups, so the barriers are
// uniform.  `red` (epilogue) and `part` (combine) are used after the loop
// only.  The empty asm statements keep the compiler from moving an LDS access
// across s_barrier, which is no memory operation to it.
//
// n_dev (live_rows.h contract): rows at or past the count supply zero codes,
// their x is never read, and their y is exactly 0.
//
// Resources (-Rpass-analysis=kernel-resource-usage, gfx950): see
// profiles/skinny_mx4_scoring.md; scratch is 0 for the three instantiations.
#include <ATen/cuda/CUDAContext.h>
#include <hip/hip_runtime.h>
#include <torch/extension.h>

#include "host_checks.h"
#include "live_rows.h"
#include "mfma_tile.h"
#include "mlp_fused.h"  // sx_a_block, sk_head, sk_combine, SK_* shared

constexpr int SX_COLS = 16;   // output columns of a workgroup
constexpr int SX_AHEAD = 8;   // chunks of a wave per K group
constexpr int SX_GK = SK_WAVES * SX_AHEAD * SK_CHUNK;  // 4096 k per group
constexpr int SX_MAX_M = 64;
constexpr int SX_TILE = 256;  // K-tile of the scale layout

// One workgroup per CU = one wave per SIMD, as in mlp_skinny.hip: the
// compiler is told not to trade registers for an occupancy the grid never
// reaches.
template <int RF>
__global__ __launch_bounds__(SK_THREADS)
__attribute__((amdgpu_waves_per_eu(1, 1))) void mlp_skinny_mx4_kernel(
    const float* __restrict__ x, float mu, float sigma,
    const bf16_t* __restrict__ w1, const bf16_t* __restrict__ b1,
    const unsigned char* __restrict__ W2q,
    const unsigned char* __restrict__ W2s, const float* __restrict__ b2,
    const float* __restrict__ w3, const float* __restrict__ b3,
    const int64_t* __restrict__ n_live, float* __restrict__ ws,
    unsigned int* __restrict__ ticket, float* __restrict__ y, int m, int H) {
  static_assert(RF == 1 || RF == 2 || RF == 4, "1, 2 or 4 row fragments");
  // [wave][fragment*4 + reg][lane]; reused by the finalise
  __shared__ float red[SK_WAVES][RF * 4][64];
  __shared__ unsigned int drawn;
  __shared__ bf16_t s_w1[SX_GK];
  __shared__ bf16_t s_b1[SX_GK];

  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int fl = lane & 15;
  const int kg = lane >> 4;
  const int n0 = blockIdx.x * SX_COLS;
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

  constexpr int PIECES = SX_GK / 8 / SK_THREADS;  // 16-byte pieces per thread
  const int nchunks = H / SK_CHUNK;
  const int nt = H / SX_TILE;
  // this lane's 16 bytes of chunk 0, and its scale dword of K-tile 0
  const unsigned char* qrow =
      W2q + (long long)(n0 + fl) * (H >> 1) + kg * 16;
  const unsigned char* srow =
      W2s + ((long long)(n0 >> 6) * nt * 64 + lane) * 8 + (wave & 1) * 4;
  const int sshift = ((n0 >> 4) & 3) * 8;

  // One group, in straight-line phases as in mlp_skinny.hip: request w1/b1,
  // request the weights and their scales, pass w1/b1 to the other waves
  // through LDS, evaluate and quantise layer 1 while the weights travel,
  // multiply.  A chunk past the end takes a valid address (chunk 0) and a
  // zero A operand.
  for (int kb = 0; kb < H; kb += SX_GK) {
    bf16x8 w1g[PIECES], b1g[PIECES];
#pragma unroll
    for (int p = 0; p < PIECES; ++p) {
      const int k = kb + (p * SK_THREADS + (int)threadIdx.x) * 8;
      if (k < H) {
        w1g[p] = load_bf16x8(w1 + k);
        b1g[p] = load_bf16x8(b1 + k);
      }
    }
    sx_i32x4 wq[SX_AHEAD];
    unsigned int wsc[SX_AHEAD];
    unsigned int keep[SX_AHEAD];
#pragma unroll
    for (int u = 0; u < SX_AHEAD; ++u) {
      const int c = kb / SK_CHUNK + u * SK_WAVES + wave;
      keep[u] = c < nchunks ? ~0u : 0u;
      const int cc = c < nchunks ? c : 0;
      wq[u] = *(const sx_i32x4*)(qrow + cc * (SK_CHUNK / 2));
      wsc[u] = *(const unsigned int*)(srow + (long long)(cc >> 1) * 512);
    }
    if (kb) {
      // see the file header: every wave has read the last group's w1/b1
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
    sx_i32x4 aq[SX_AHEAD][RF];
    int asc[SX_AHEAD][RF];
#pragma unroll
    for (int u = 0; u < SX_AHEAD; ++u) {
      // the same 32 k as wq[u], relative to the group
      const int c8 = (u * SK_WAVES + wave) * (SK_CHUNK / 8) + kg * 4;
#pragma unroll
      for (int r = 0; r < RF; ++r)
        aq[u][r] = sx_a_block(xn[r], alive[r] ? keep[u] : 0u, s_w1, s_b1, c8,
                              asc[u][r]);
    }
#pragma unroll
    for (int u = 0; u < SX_AHEAD; ++u) {
      const int bsc = (int)((wsc[u] >> sshift) & 0xFFu);
#pragma unroll
      for (int r = 0; r < RF; ++r)
        acc[r] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
            sx_operand(aq[u][r]), sx_operand(wq[u]), acc[r], SX_FMT, SX_FMT,
            0, asc[u][r], 0, bsc);
    }
  }

  // the four K-slices added in wave order, +b2, relu, *w3, 16 columns summed
  sk_head<RF>(acc, &red[0][0][0], b2, w3, ws, n0, wave, lane);
  // ticket: the last workgroup to arrive adds up the partials (red was last
  // read in sk_head)
  sk_combine<RF>(wave < RF, RF, &red[0][0][0], &drawn, ws, ticket, b3, y, m,
                 live);
}

// ---- host side --------------------------------------------------------------

at::Tensor mlp_skinny_score_mxfp4_hip(
    const at::Tensor& x, double mu, double sigma, const at::Tensor& w1,
    const at::Tensor& b1, const at::Tensor& w2q, const at::Tensor& w2s,
    const at::Tensor& b2, const at::Tensor& w3, const at::Tensor& b3,
    const c10::optional<at::Tensor>& n_dev) {
  const char* op = "mlp_skinny_score_mxfp4";
  const MlpScoreOperands a =
      mlp_score_vectors(op, SX_MAX_M, SX_TILE, x, w1, b1, b2, w3, b3);
  const int64_t m = a.m, H = a.H;
  TORCH_CHECK(w2q.dim() == 2 && w2q.size(0) == H && w2q.size(1) == H / 2, op,
              ": w2q must be [H, H/2] = the codes of the [out, in] matrix");
  const void* q = mlp_score_operand(op, "w2q", w2q, x, at::kByte, H * H / 2);
  const void* s = mlp_score_operand(op, "w2s", w2s, x, at::kByte, H * H / 32);
  TORCH_CHECK((uintptr_t)q % 16 == 0 && (uintptr_t)s % 8 == 0 &&
                  (uintptr_t)a.w1 % 16 == 0 && (uintptr_t)a.b1 % 16 == 0,
              op, ": w2q, w1 and b1 must be 16-byte and w2s 8-byte aligned");
  const int64_t* n_live = n_live_ptr(n_dev, x, op);

  const int rf = m <= 16 ? 1 : (m <= 32 ? 2 : 4);
  const int grid = (int)(H / SX_COLS);
  // fresh on every call (under capture: from the graph's pool, the zero
  // fill replayed with the graph), so there is no state to reset
  auto ws = at::empty({grid, 16 * rf}, x.options());
  auto ticket = at::zeros({1}, x.options().dtype(at::kInt));
  auto y = at::empty({m}, x.options());
  auto stream = at::cuda::getCurrentCUDAStream();
#define SX_LAUNCH(RF_)                                                       \
  hipLaunchKernelGGL((mlp_skinny_mx4_kernel<RF_>), dim3(grid),               \
                     dim3(SK_THREADS), 0, stream, x.data_ptr<float>(),       \
                     (float)mu, (float)sigma, (const bf16_t*)a.w1,           \
                     (const bf16_t*)a.b1, (const unsigned char*)q,           \
                     (const unsigned char*)s, a.b2, a.w3, a.b3, n_live,      \
                     ws.data_ptr<float>(),                                   \
                     (unsigned int*)ticket.data_ptr<int>(),                  \
                     y.data_ptr<float>(), (int)m, (int)H)
  if (rf == 1) SX_LAUNCH(1);
  else if (rf == 2) SX_LAUNCH(2);
  else SX_LAUNCH(4);
#undef SX_LAUNCH
  return y;
}
