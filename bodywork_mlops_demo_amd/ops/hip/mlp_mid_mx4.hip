// Mini-batch MLP scoring on MXFP4 operands: the forward of 1..256 rows in a
// PAIR of kernels, the arithmetic of mlp_skinny_mx4.hip:
//
//   y[m] = b3 + sum_n w3[n] * relu(b2[n] + sum_k dq(W2)[n,k] * dq(h1)[m,k])
//   h1[m,k] = relu(xn[m] * w1[k] + b1[k]) in fp32,  xn = (x - mu) / sigma
//
// dq(.) is the MXFP4 decode; W2 arrives quantised (ops.quantize_mxfp4), h1 is
// quantised here to the bits ops.expand1d_mxfp4 writes (sx_a_block,
// mlp_fused.h: the quantiser's own arithmetic).
//
// Why two kernels.  mlp_mid.hip evaluates layer 1 in every column workgroup
// and is bound by that VALU work; the fp4 quantiser (block amax, exponent,
// scaled convert) makes a fragment several times dearer while the fp4 MFMA
// that consumes it is one instruction per K = 128.  So layer 1 is quantised
// ONCE, by a stage kernel, into a small buffer that stays in cache, and the
// head kernel's A operand is a plain load.  The kernel boundary is the only
// ordering between the two: no workgroup waits on another.
//
// Staging buffer (private to this file, ordered for the consumer).  With
// nchunks = H/128, row fragment r (16 rows), chunk c (128 k):
//  * codes: the 64 16-byte operands of (r, c) in lane order, 1 KiB at
//      ((r*nchunks + c)*64 + lane)*16,
//    lane (fl, kg) = row 16r+fl, 32-block 4c+kg: the MFMA's A operand as it
//    is.  One wave's A load of (r, c) is one contiguous 1 KiB burst.
//  * scales: one dword per (c, block of four fragments g, lane) at
//      ((c*4 + g)*64 + lane)*4,   byte r&3 = the E8M0 byte of fragment 4g+(r&3)
//    so one 256-byte burst serves four fragments and the byte is picked by the
//    MFMA's op_sel (a literal: the fragment loop is unrolled).
//  512 KiB + 32 KiB at H = 4096.
//
// Stage kernel: one wave per (r, c), two waves per workgroup, grid (nchunks/2,
// ceil(m/16)).  A lane evaluates and quantises its own 32-block from w1/b1 in
// global memory (8 16-byte loads, cache hits) and stores 16 bytes and one
// byte.  Fragments at or past ceil(live/16) are not written; inside a live
// fragment a row at or past the count gets zero codes and byte 127 and its x
// is never read.  Thread 0 of workgroup (0, 0) zeroes the combine ticket,
// which replaces the fill node of the other one-kernel paths.
//
// Head kernel, the skeleton of mlp_mid.hip:
//  * one workgroup (4 waves) owns 16*CF = 32 output columns, grid = H/32; the
//    full K stays inside it, wave w takes chunks w, w+4, ...
//  * B operand: codes and the scale dword from global memory straight into
//    operand registers as in mlp_skinny_mx4.hip (one 16-byte load per lane,
//    chunk and column fragment).  The two column fragments of a workgroup lie
//    in one 64-row scale group, so ONE dword holds both bytes; each is
//    shifted to position 0.
//  * A operand: the loads above; no VALU, no LDS.
//  * the accumulators of ALL live row fragments stay in registers for the
//    whole K slice (16 x CF x 4 = 128 at 256 rows), so nothing goes through
//    LDS between K groups.
//  * schedule: the chunk loop is rolled and walks two chunk buffers; the loads
//    of chunk i+1 are issued ahead of the MFMAs of chunk i, so a load has the
//    MFMAs of one chunk (8 per block of four fragments, CF = 2) to land.  All
//    loads of a buffer are unconditional and in one order, so the compiler's
//    vmcnt ahead of an MFMA counts exactly the loads behind its operands and
//    leaves the next chunk's in flight (at most 46 are outstanding).
//  * live count: the kernel body is built for NQ = 1..4 blocks of four
//    fragments and chosen by ceil(nfrag/4), a scalar.  Inside the last block
//    a fragment past the count takes the address of the last live fragment
//    (nothing unwritten is read) and its MFMAs are skipped by a scalar test,
//    outside any barrier.  Loads and MFMAs are proportional to the live
//    fragments; the weight stream is not.
//  * epilogue, as mlp_mid.hip writes it: accumulators to LDS, the four K
//    slices added in wave order, +b2, relu, *w3, the column fragments in
//    order, a butterfly over 16 columns; ws is [grid, 256]; sk_combine<16>.
//
// Every row's sum has one fixed order (chunks of a wave, waves, column
// fragments, columns, workgroups), whatever m, the count or the other rows
// are: bitwise reproducible and row-independent.
//
// Resources (-Rpass-analysis=kernel-resource-usage, gfx950): see
// profiles/mid_mx4_scoring.md; scratch is 0 for both kernels.
#include <ATen/cuda/CUDAContext.h>
#include <hip/hip_runtime.h>
#include <torch/extension.h>

#include <utility>

#include "host_checks.h"
#include "live_rows.h"
#include "mfma_tile.h"
#include "mlp_fused.h"  // sx_a_block, sx_operand, sk_combine, SK_* shared

constexpr int MM_MAX_M = 256;
constexpr int MM_FRAGS = MM_MAX_M / 16;
constexpr int MM_CF = 2;             // column fragments of a head workgroup
constexpr int MM_TILE = 256;         // K-tile of the scale layout
constexpr int MM_STAGE_THREADS = 128;  // two (fragment, chunk) pairs

// byte offsets into the staging buffer, lane 0
__device__ __forceinline__ long long mm_code_offset(int r, int c,
                                                    int nchunks) {
  return ((long long)r * nchunks + c) * 1024;
}
__device__ __forceinline__ long long mm_scale_offset(int g, int c) {
  return ((long long)c * 4 + g) * 256;
}

// ---- kernel 1: layer 1, quantised once --------------------------------------
__global__ __launch_bounds__(MM_STAGE_THREADS) void mlp_mid_mx4_stage_kernel(
    const float* __restrict__ x, float mu, float sigma,
    const bf16_t* __restrict__ w1, const bf16_t* __restrict__ b1,
    const int64_t* __restrict__ n_live, unsigned char* __restrict__ stage_q,
    unsigned char* __restrict__ stage_s, unsigned int* __restrict__ ticket,
    int m, int H) {
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int fl = lane & 15;
  const int kg = lane >> 4;
  const int r = blockIdx.y;
  const int c = blockIdx.x * 2 + wave;  // H % 256 == 0: both waves have one
  const int live = n_live ? (int)live_count(n_live, m) : m;

  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *ticket = 0u;
  if (r * 16 >= live) return;  // block-uniform

  const int row = r * 16 + fl;
  const bool alive = row < live;
  const float xn = alive ? (x[row] - mu) / sigma : 0.0f;
  int scale;
  const sx_i32x4 q = sx_a_block(xn, alive ? ~0u : 0u, w1, b1,
                                c * (SK_CHUNK / 8) + kg * 4, scale);
  *(sx_i32x4*)(stage_q + mm_code_offset(r, c, H / SK_CHUNK) + lane * 16) = q;
  stage_s[mm_scale_offset(r >> 2, c) + lane * 4 + (r & 3)] =
      (unsigned char)scale;
}

// ---- kernel 2: weight stream, MFMA, head ------------------------------------

// the operands of one chunk of one wave, NR row fragments
template <int NR>
struct MmChunk {
  sx_i32x4 a[NR];
  unsigned int as[NR / 4];
  sx_i32x4 b[MM_CF];
  unsigned int bs;
};

// where a wave's operands of chunk 0 are
struct MmBase {
  const unsigned char* aq;  // staging codes + lane*16
  const unsigned char* as;  // staging scales + lane*4
  const unsigned char* bq;  // W2 codes: row n0+fl, + kg*16
  const unsigned char* bs;  // W2 scale dword of this lane, parity of the wave
  long long bq_cf;          // bytes between the column fragments: 16 rows
  int nchunks, nfrag, bshift;
};

// every load of chunk c, unconditional: B first (the farthest memory)
template <int NR>
__device__ __forceinline__ void mm_load(MmChunk<NR>& k, const MmBase& p,
                                        int c) {
#pragma unroll
  for (int cf = 0; cf < MM_CF; ++cf)
    k.b[cf] = *(const sx_i32x4*)(p.bq + cf * p.bq_cf + c * (SK_CHUNK / 2));
  k.bs = *(const unsigned int*)(p.bs + (long long)(c >> 1) * 512);
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    // a fragment past the count: the last live one's, never multiplied
    const int rr = min(r, p.nfrag - 1);
    k.a[r] = *(const sx_i32x4*)(p.aq + mm_code_offset(rr, c, p.nchunks));
  }
#pragma unroll
  for (int g = 0; g < NR / 4; ++g)
    k.as[g] = *(const unsigned int*)(p.as + mm_scale_offset(g, c));
}

// fragment R of a chunk times both column fragments; op_sel has to be a
// literal, hence the template parameter
template <int NR, int R>
__device__ __forceinline__ void mm_frag(f32x4 (&acc)[NR][MM_CF],
                                        const MmChunk<NR>& k, int nfrag,
                                        int bshift) {
  if (R < nfrag) {  // wave-uniform
#pragma unroll
    for (int cf = 0; cf < MM_CF; ++cf)
      acc[R][cf] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
          sx_operand(k.a[R]), sx_operand(k.b[cf]), acc[R][cf], SX_FMT, SX_FMT,
          R & 3, (int)k.as[R >> 2], 0,
          (int)((k.bs >> (bshift + 8 * cf)) & 0xFFu));
  }
}

template <int NR, int... R>
__device__ __forceinline__ void mm_mfma(f32x4 (&acc)[NR][MM_CF],
                                        const MmChunk<NR>& k, const MmBase& p,
                                        std::integer_sequence<int, R...>) {
  (mm_frag<NR, R>(acc, k, p.nfrag, p.bshift), ...);
}

// the K slice of one wave for NQ blocks of four row fragments; the
// accumulators end in red[wave][fragment][column fragment][reg][lane]
template <int NQ>
__device__ __forceinline__ void mm_k_slice(const MmBase& p, int wave,
                                           int lane, float* red_wave) {
  constexpr int NR = 4 * NQ;
  const auto frags = std::make_integer_sequence<int, NR>{};
  f32x4 acc[NR][MM_CF];
#pragma unroll
  for (int r = 0; r < NR; ++r)
#pragma unroll
    for (int cf = 0; cf < MM_CF; ++cf)
      acc[r][cf] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

  // chunks wave, wave+4, ...: `even` holds chunk c on entry to the loop body
  // and to the tail; every branch is wave-uniform
  MmChunk<NR> even, odd;
  int c = wave;
  if (c < p.nchunks) {
    mm_load(even, p, c);
#pragma unroll 1
    for (; c + 2 * SK_WAVES < p.nchunks; c += 2 * SK_WAVES) {
      mm_load(odd, p, c + SK_WAVES);
      mm_mfma(acc, even, p, frags);
      mm_load(even, p, c + 2 * SK_WAVES);
      mm_mfma(acc, odd, p, frags);
    }
    if (c + SK_WAVES < p.nchunks) {
      mm_load(odd, p, c + SK_WAVES);
      mm_mfma(acc, even, p, frags);
      mm_mfma(acc, odd, p, frags);
    } else {
      mm_mfma(acc, even, p, frags);
    }
  }

#pragma unroll
  for (int r = 0; r < NR; ++r)
    if (r < p.nfrag) {
#pragma unroll
      for (int cf = 0; cf < MM_CF; ++cf)
#pragma unroll
        for (int q = 0; q < 4; ++q)
          red_wave[((r * MM_CF + cf) * 4 + q) * 64 + lane] = acc[r][cf][q];
    }
}

// One workgroup per CU = one wave per SIMD, as in mlp_mid.hip: the whole
// register file is a wave's.
__global__ __launch_bounds__(SK_THREADS)
__attribute__((amdgpu_waves_per_eu(1, 1))) void mlp_mid_mx4_head_kernel(
    const unsigned char* __restrict__ stage_q,
    const unsigned char* __restrict__ stage_s,
    const unsigned char* __restrict__ W2q,
    const unsigned char* __restrict__ W2s, const float* __restrict__ b2,
    const float* __restrict__ w3, const float* __restrict__ b3,
    const int64_t* __restrict__ n_live, float* __restrict__ ws,
    unsigned int* __restrict__ ticket, float* __restrict__ y, int m, int H) {
  constexpr int CF = MM_CF;
  // [wave][fragment][column fragment][reg][lane]; reused by the combine
  __shared__ float red[SK_WAVES][MM_FRAGS][CF][4][64];
  __shared__ unsigned int drawn;

  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int fl = lane & 15;
  const int kg = lane >> 4;
  const int n0 = blockIdx.x * (16 * CF);
  const int live = n_live ? (int)live_count(n_live, m) : m;
  const int nfrag = (live + 15) >> 4;

  MmBase p;
  p.nchunks = H / SK_CHUNK;
  p.nfrag = nfrag;
  p.aq = stage_q + lane * 16;
  p.as = stage_s + lane * 4;
  p.bq = W2q + (long long)(n0 + fl) * (H >> 1) + kg * 16;
  p.bq_cf = 16LL * (H >> 1);
  // mx4_scale_index of row n0 + 16*cf + fl, block 4c + kg: the dword (c & 1 =
  // wave & 1) of this lane in K-tile c >> 1, byte ((n0 >> 4) & 3) + cf
  p.bs = W2s + ((long long)(n0 >> 6) * (H / MM_TILE) * 64 + lane) * 8 +
         (wave & 1) * 4;
  p.bshift = ((n0 >> 4) & 3) * 8;

  float* red_wave = &red[wave][0][0][0][0];
  const int nq = (nfrag + 3) >> 2;  // block-uniform
  if (nq == 1) mm_k_slice<1>(p, wave, lane, red_wave);
  else if (nq == 2) mm_k_slice<2>(p, wave, lane, red_wave);
  else if (nq == 3) mm_k_slice<3>(p, wave, lane, red_wave);
  else if (nq == 4) mm_k_slice<4>(p, wave, lane, red_wave);
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
        ws[(long long)blockIdx.x * MM_MAX_M + r * 16 + kg * 4 + q] = t[q];
    }
  }

  // red was last read above; the combine's first barrier is ahead of its
  // writes
  sk_combine<MM_FRAGS>(wave < nfrag, nfrag, &red[0][0][0][0][0], &drawn, ws,
                       ticket, b3, y, m, live);
}

// ---- host side --------------------------------------------------------------

at::Tensor mlp_mid_score_mxfp4_hip(
    const at::Tensor& x, double mu, double sigma, const at::Tensor& w1,
    const at::Tensor& b1, const at::Tensor& w2q, const at::Tensor& w2s,
    const at::Tensor& b2, const at::Tensor& w3, const at::Tensor& b3,
    const c10::optional<at::Tensor>& n_dev) {
  const char* op = "mlp_mid_score_mxfp4";
  const MlpScoreOperands a =
      mlp_score_vectors(op, MM_MAX_M, MM_TILE, x, w1, b1, b2, w3, b3);
  const int64_t m = a.m, H = a.H;
  TORCH_CHECK(w2q.dim() == 2 && w2q.size(0) == H && w2q.size(1) == H / 2, op,
              ": w2q must be [H, H/2] = the codes of the [out, in] matrix");
  const void* q = mlp_score_operand(op, "w2q", w2q, x, at::kByte, H * H / 2);
  const void* s = mlp_score_operand(op, "w2s", w2s, x, at::kByte, H * H / 32);
  TORCH_CHECK((uintptr_t)q % 16 == 0 && (uintptr_t)s % 8 == 0 &&
                  (uintptr_t)a.w1 % 16 == 0 && (uintptr_t)a.b1 % 16 == 0,
              op, ": w2q, w1 and b1 must be 16-byte and w2s 8-byte aligned");
  const int64_t* n_live = n_live_ptr(n_dev, x, op);

  const int nchunks = (int)(H / SK_CHUNK);
  const int grid = (int)(H / (16 * MM_CF));
  // fresh on every call (under capture: from the graph's pool), so there is
  // no state to reset; the stage kernel zeroes the ticket
  const auto bytes = x.options().dtype(at::kByte);
  auto stage_q = at::empty({MM_FRAGS, nchunks, 1024}, bytes);
  auto stage_s = at::empty({nchunks, MM_FRAGS / 4, 256}, bytes);
  auto ws = at::empty({grid, MM_MAX_M}, x.options());
  auto ticket = at::empty({1}, x.options().dtype(at::kInt));
  auto y = at::empty({m}, x.options());
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(mlp_mid_mx4_stage_kernel,
                     dim3(nchunks / 2, (unsigned)((m + 15) / 16)),
                     dim3(MM_STAGE_THREADS), 0, stream, x.data_ptr<float>(),
                     (float)mu, (float)sigma, (const bf16_t*)a.w1,
                     (const bf16_t*)a.b1, n_live,
                     stage_q.data_ptr<unsigned char>(),
                     stage_s.data_ptr<unsigned char>(),
                     (unsigned int*)ticket.data_ptr<int>(), (int)m, (int)H);
  hipLaunchKernelGGL(mlp_mid_mx4_head_kernel, dim3(grid), dim3(SK_THREADS), 0,
                     stream, stage_q.data_ptr<unsigned char>(),
                     stage_s.data_ptr<unsigned char>(),
                     (const unsigned char*)q, (const unsigned char*)s, a.b2,
                     a.w3, a.b3, n_live, ws.data_ptr<float>(),
                     (unsigned int*)ticket.data_ptr<int>(),
                     y.data_ptr<float>(), (int)m, (int)H);
  return y;
}
