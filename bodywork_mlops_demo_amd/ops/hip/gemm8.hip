// 256x256-tile 8-phase software-pipelined NT MFMA GEMM (gfx950).
//
// The deep-pipeline variant of gemm.hip's 128^2 kernel (which sits at
// the documented plain-HIP 2-phase ceiling, ~1000 TF): 16 waves per
// 1024-thread block (4x4), per-wave C = 64x64 = 4x4 fragments; one
// K-tile (BK=64) is computed as 4 "quadrant" phases of 8 MFMAs each,
// with the operand traffic software-pipelined at HALF-TILE (16 KiB)
// granularity:
//
//   phase (u,q):  [q==0: s_waitcnt vmcnt(4), or vmcnt(0) on the last
//                  tile]                        <- once per K-tile
//                 s_barrier                     <- ONE barrier per phase
//                 issue glds (schedule below; one wave-level glds
//                   instruction per half-tile at 1024 threads)
//                 ds_read this quadrant's A fragments (2x b128) feeding
//                   the SAME phase's MFMAs [q==0: + ALL of tile u's B
//                   fragments (8); q==2: + quadrant 3 pre-read]
//                 s_setprio(1); 8 x mfma_f32_16x16x32_bf16; s_setprio(0)
//
// Issue schedule:
//   (u,1): B0(u+2)   (u,2): B1(u+2)   (u,3): A0(u+2)+A1(u+2)
// Landing proof: at (u,0) the four newest outstanding glds are tile
// u+1's {B0,B1,A0,A1}; the 5th-newest is tile u's A1 -> vmcnt(4) proves
// tile u fully landed while keeping the pipeline 4 deep (never drains;
// the final tile, with no newer issues, drains with vmcnt(0) once).
// Slot-reuse safety: every glds overwrites a slot whose last ds_read
// happened in an EARLIER phase, separated by a barrier — B(u) slots are
// read only at (u,0) and re-staged at (u,1)/(u,2); A(u) slots are last
// read at (u,2) (quadrant 3 pre-reads there) and re-staged at (u,3).
//
// LDS: per operand 2 buffers x 2 halves x [128][64] shorts = 64 KiB;
// A+B = 128 KiB -> 1 block/CU, 16 waves (4/SIMD, so the per-lane VGPR
// cap is 128).  Measured allocation: 124-126 VGPR, ZERO spills (acc 64 +
// B 32 + A 2x8 + addressing) — unlike the earlier 8-wave/128-row-per-wave
// variant which hit the 256 cap with spills.
// Same 16-byte-chunk XOR swizzle as gemm.hip, carried on the glds SOURCE
// address and the fragment read.  The K-loop is unrolled two tiles per
// iteration so every register-set index is compile-time (rule 20).
//
// Requirements: M % 256 == 0, N % 256 == 0, K % 128 == 0 (dispatched for
// those shapes only; others use the 128^2 kernel).  DEFAULT path for
// qualifying shapes — A/B-measured 1249-1292 TF vs the 128^2 kernel's
// 1011-1084 (same box, profiles/r01_gemm_variant_study.md);
// BODYWORK_GEMM_8PHASE=0 opts out.  An 8-wave variant and a bf16 port of
// gemm_mx8.hip's single-phase schedule both measured 1-3% behind this
// kernel and were removed (docs/GEMM_DESIGN.md; last present at 850e461).
#include <ATen/cuda/CUDAContext.h>
#include <hip/hip_runtime.h>
#include <torch/extension.h>

#include <type_traits>

#include "bf16_utils.h"
#include "host_checks.h"
#include "mfma_tile.h"

#define G8_BM 256
#define G8_BN 256
#define G8_BK 64
#define G8_THREADS 1024
#define G8_HT (128 * 64)  // shorts per half-tile slot

// The epilogue's read-only operand rides in ONE kernel-argument slot typed by
// the mode: w3 (fp32 [N]) for the fused scoring head, else the 1-bit mask.
template <Epi EPI>
using EpiOperand = std::conditional_t<EPI == Epi::ReluDot, const float*,
                                      const unsigned char*>;

// stage one [128][64]-bf16 half-tile: 1024 16-B chunks, 1024 threads ->
// ONE wave-level glds per wave.  Lane-linear LDS; XOR swizzle on the
// source.  The per-lane source BYTE offset (row*K + swizzled column
// chunk) is tile-invariant — computed once at kernel entry (32-bit), so
// the hot loop's staging is {uniform base + int offset} with no 64-bit
// per-lane math (this kernel is dispatched only for M,N % 256 == 0, so
// no row clamping is needed).
__device__ __forceinline__ void g8_stage_half(short* __restrict__ slot,
                                              const char* __restrict__ base,
                                              int off0) {
  const int wave = threadIdx.x >> 6;
  glds16(base + off0, (char*)slot + wave * 1024);
}

// LIVE (the scoring head only): row tiles at or past the device-side live
// row count return at once and rows at or past it add nothing to y (same
// contract as gemm_mx8.hip's head).
template <Epi EPI, bool HAS_BIAS, bool OUT_FP32, bool EMIT_MASK = false,
          bool LIVE = false>
__launch_bounds__(G8_THREADS)
__global__ void gemm_nt_8phase_kernel(
    const bf16_t* __restrict__ A,  // [M,K]
    const bf16_t* __restrict__ B,  // [N,K]
    const float* __restrict__ bias, EpiOperand<EPI> __restrict__ epi_in,
    unsigned char* __restrict__ mask_out, void* __restrict__ C, long long M,
    long long N, long long K,
    const int64_t* __restrict__ n_live = nullptr) {  // LIVE only
  // ONE __shared__ object (guide §5 trap (a))
  __shared__ short lds[8 * G8_HT];  // [op A=0/B=1][buf][half][128][64]
  const long long m0 = (long long)blockIdx.y * G8_BM;
  int live_rows = G8_BM;
  if constexpr (LIVE) {
    static_assert(EPI == Epi::ReluDot, "live rows: scoring head only");
    if (!tile_live_rows<G8_BM>(n_live, M, m0, live_rows)) return;
  }
  const long long n0 = (long long)blockIdx.x * G8_BN;
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int wm = wave >> 2;  // 0..3 (64 C-rows per wave)
  const int wn = wave & 3;   // 0..3 (64 C-cols per wave)
  const int fl = lane & 15;
  const int kg = lane >> 4;
  const int swz = fl & 7;
  const long long nt = K / G8_BK;

  // slot base (in shorts): op*4HT + buf*2HT + half*HT
#define G8_ASLOT(buf, half) (lds + ((buf) * 2 + (half)) * G8_HT)
#define G8_BSLOT(buf, half) (lds + 4 * G8_HT + ((buf) * 2 + (half)) * G8_HT)

  // wave-local read bases: this wave only touches A-half (wm>>1) and
  // B-half (wn>>1); within-half row offsets are compile-time
  const int a_inhalf = (wm & 1) * 64;
  const int b_inhalf = (wn & 1) * 64;

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

#define G8_AREAD(dst, buf, mfrag, ks)                                       \
  dst = ((const lds_vec*)(G8_ASLOT(buf, (wm >> 1)) +                        \
                          (a_inhalf + (mfrag) * 16 + fl) * 64 +             \
                          (((ks) * 4 + kg) ^ swz) * 8))                     \
            ->v
#define G8_BREAD(dst, buf, nfrag, ks)                                       \
  dst = ((const lds_vec*)(G8_BSLOT(buf, (wn >> 1)) +                        \
                          (b_inhalf + (nfrag) * 16 + fl) * 64 +             \
                          (((ks) * 4 + kg) ^ swz) * 8))                     \
            ->v

  bf16x8_v a_q[2];     // current quadrant's A fragments [ks]
  bf16x8_v a_q3[2];    // quadrant 3, pre-read one phase early (slot-free proof)
  bf16x8_v b_t[4][2];  // current tile's B fragments [nfrag][ks]

  // per-lane staging byte offset (tile-invariant; see g8_stage_half)
  int stg_off;
  {
    int ci = (int)threadIdx.x;
    int row = ci >> 3;
    int sc = (ci & 7) ^ (row & 7);
    stg_off = (int)((row * K + sc * 8) * 2);
  }
  const char* Ah0 = (const char*)(A + m0 * K);
  const char* Ah1 = (const char*)(A + (m0 + 128) * K);
  const char* Bh0 = (const char*)(B + n0 * K);
  const char* Bh1 = (const char*)(B + (n0 + 128) * K);
#define G8_KOFF(T) ((long long)(T) * (G8_BK * 2))

  // ---- prologue: A(0), B(0), B(1) (6 half-tiles; A(1) is issued by the
  // loop at phase (0,A)).  At the first wait `vmcnt(2)` keeps the newest
  // two (tile 1's B halves) in flight and proves tile 0 landed.
  g8_stage_half(G8_ASLOT(0, 0), Ah0, stg_off);
  g8_stage_half(G8_ASLOT(0, 1), Ah1, stg_off);
  g8_stage_half(G8_BSLOT(0, 0), Bh0, stg_off);
  g8_stage_half(G8_BSLOT(0, 1), Bh1, stg_off);
  if (nt > 1) {
    g8_stage_half(G8_BSLOT(1, 0), Bh0 + G8_KOFF(1), stg_off);
    g8_stage_half(G8_BSLOT(1, 1), Bh1 + G8_KOFF(1), stg_off);
  }

  // One phase = barrier + (issue) + LDS reads + 8 MFMAs.  Reads feed the
  // SAME phase's MFMAs (lgkm waits are in-phase), except quadrant 3 which
  // is pre-read at phase 2 so that phase 3's A-slot glds issues target a
  // slot with no reads outstanding.  Issue/wait schedule per tile u:
  //   (u,0): s_waitcnt vmcnt(4); read B(u) x8 + A q0; MFMA q0
  //   (u,1): issue B0(u+2);      read A q1;           MFMA q1
  //   (u,2): issue B1(u+2);      read A q2 AND q3;    MFMA q2
  //   (u,3): issue A0,A1(u+2);                        MFMA q3
  // Landing proof: at (u,0) the newest 4 outstanding glds are tile u+1's
  // {B0,B1,A0,A1}; the 5th-newest is A1(u) -> vmcnt(4) proves all of tile
  // u landed.  Slot-free proof: every glds targets a slot whose last
  // ds_read happened in an EARLIER phase (barrier-separated): B(u) slots
  // read only at (u,0), re-staged at (u,1)/(u,2); A(u) slots last read at
  // (u,2) (q3 pre-read), re-staged at (u,3).
// Two 32-MFMA phases per K-tile (v4): half the barriers of the
// 4-phase schedule.  Phase A: wait+barrier, issue A(T+1), first-touch
// reads of B(T) x8 + A q0,q1, MFMA q0+q1 (16).  Phase B: barrier,
// issue B(T+2), read A q2,q3, MFMA q2+q3 (16).
// Landing: at wait(T,A) the newest 2 outstanding glds are B(T+1)'s
// halves (issued at (T-1,B)); the 3rd/4th-newest are A(T)'s halves
// (issued at (T-1,A)) -> vmcnt(2) proves tile T landed; the last tile
// drains with vmcnt(0).  Slot safety is completion-airtight: A(T+1)
// overwrites A(T-1), whose q2/q3 reads were CONSUMED by MFMAs before
// any wave passed barrier(T,A); B(T+2) overwrites B(T), whose reads
// were consumed by MFMA q0/q1 before barrier(T,B).
#define G8_PHASE_A(T, TPAR)                                                 \
  do {                                                                      \
    if ((T) + 1 < nt)                                                       \
      asm volatile("s_waitcnt vmcnt(2)" ::: "memory");                      \
    else                                                                    \
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                      \
    __builtin_amdgcn_s_barrier();                                           \
    if ((T) + 1 < nt) {                                                     \
      g8_stage_half(G8_ASLOT(1 - (TPAR), 0), Ah0 + G8_KOFF((T) + 1),        \
                    stg_off);                                               \
      g8_stage_half(G8_ASLOT(1 - (TPAR), 1), Ah1 + G8_KOFF((T) + 1),        \
                    stg_off);                                               \
    }                                                                       \
    _Pragma("unroll") for (int nf = 0; nf < 4; ++nf) {                      \
      G8_BREAD(b_t[nf][0], TPAR, nf, 0);                                    \
      G8_BREAD(b_t[nf][1], TPAR, nf, 1);                                    \
    }                                                                       \
    G8_AREAD(a_q[0], TPAR, 0, 0);                                           \
    G8_AREAD(a_q[1], TPAR, 0, 1);                                           \
    G8_AREAD(a_q3[0], TPAR, 1, 0);                                          \
    G8_AREAD(a_q3[1], TPAR, 1, 1);                                          \
    __builtin_amdgcn_s_setprio(1);                                          \
    _Pragma("unroll") for (int nf = 0; nf < 4; ++nf)                        \
        _Pragma("unroll") for (int ks = 0; ks < 2; ++ks)                    \
            acc[0][nf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(           \
                a_q[ks], b_t[nf][ks], acc[0][nf], 0, 0, 0);                 \
    _Pragma("unroll") for (int nf = 0; nf < 4; ++nf)                        \
        _Pragma("unroll") for (int ks = 0; ks < 2; ++ks)                    \
            acc[1][nf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(           \
                a_q3[ks], b_t[nf][ks], acc[1][nf], 0, 0, 0);                \
    __builtin_amdgcn_s_setprio(0);                                          \
  } while (0)

#define G8_PHASE_B(T, TPAR)                                                 \
  do {                                                                      \
    __builtin_amdgcn_s_barrier();                                           \
    if ((T) + 2 < nt) {                                                     \
      g8_stage_half(G8_BSLOT(TPAR, 0), Bh0 + G8_KOFF((T) + 2), stg_off);    \
      g8_stage_half(G8_BSLOT(TPAR, 1), Bh1 + G8_KOFF((T) + 2), stg_off);    \
    }                                                                       \
    G8_AREAD(a_q[0], TPAR, 2, 0);                                           \
    G8_AREAD(a_q[1], TPAR, 2, 1);                                           \
    G8_AREAD(a_q3[0], TPAR, 3, 0);                                          \
    G8_AREAD(a_q3[1], TPAR, 3, 1);                                          \
    __builtin_amdgcn_s_setprio(1);                                          \
    _Pragma("unroll") for (int nf = 0; nf < 4; ++nf)                        \
        _Pragma("unroll") for (int ks = 0; ks < 2; ++ks)                    \
            acc[2][nf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(           \
                a_q[ks], b_t[nf][ks], acc[2][nf], 0, 0, 0);                 \
    _Pragma("unroll") for (int nf = 0; nf < 4; ++nf)                        \
        _Pragma("unroll") for (int ks = 0; ks < 2; ++ks)                    \
            acc[3][nf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(           \
                a_q3[ks], b_t[nf][ks], acc[3][nf], 0, 0, 0);                \
    __builtin_amdgcn_s_setprio(0);                                          \
  } while (0)

  // two tiles per iteration: buffer indices stay compile-time (rule 20)
  for (long long t = 0; t < nt; t += 2) {
    G8_PHASE_A(t, 0);
    G8_PHASE_B(t, 0);
    if (t + 1 < nt) {
      G8_PHASE_A(t + 1, 1);
      G8_PHASE_B(t + 1, 1);
    }
  }
#undef G8_PHASE_A
#undef G8_PHASE_B
#undef G8_AREAD
#undef G8_BREAD
#undef G8_ASLOT
#undef G8_BSLOT

  const float* w3 = nullptr;
  const unsigned char* mask = nullptr;
  if constexpr (EPI == Epi::ReluDot) w3 = epi_in;
  else mask = epi_in;
  tile_epilogue<EPI, HAS_BIAS, OUT_FP32, EMIT_MASK, LIVE>(
      acc, bias, w3, mask, mask_out, C, M, N, m0, n0, wm, wn, fl, kg,
      live_rows);
}

// y[M] = sum_col relu(x.w^T + b2) * w3 — the bf16 MLP scoring forward's
// h2 GEMM and rowdot head in ONE kernel (the [M,N] activation tensor
// never reaches HBM).  Caller adds b3.  With n_dev (int64[1] on x's
// device) the row tiles past that live count return at once and
// y[n_dev:] stays 0.
at::Tensor gemm8_relu_dot_bf16_hip(const at::Tensor& x, const at::Tensor& w,
                                   const at::Tensor& b2, const at::Tensor& w3,
                                   const c10::optional<at::Tensor>& n_dev) {
  TORCH_CHECK(x.is_cuda() && w.is_cuda() && x.dim() == 2 && w.dim() == 2 &&
                  x.size(1) == w.size(1),
              "gemm8_relu_dot: [M,K]x[N,K] cuda");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 &&
              w.scalar_type() == at::kBFloat16);
  TORCH_CHECK(x.is_contiguous() && w.is_contiguous());
  long long M = x.size(0), K = x.size(1), N = w.size(0);
  TORCH_CHECK(M % G8_BM == 0 && N % G8_BN == 0 && K % (2 * G8_BK) == 0,
              "gemm8_relu_dot requires M%256==0, N%256==0, K%128==0");
  TORCH_CHECK(b2.is_cuda() && b2.scalar_type() == at::kFloat &&
                  b2.numel() == N, "b2: fp32 [N]");
  TORCH_CHECK(w3.is_cuda() && w3.scalar_type() == at::kFloat &&
                  w3.numel() == N, "w3: fp32 [N]");
  const int64_t* n_live = n_live_ptr(n_dev, x, "gemm8_relu_dot");
  auto y = at::zeros({M}, x.options().dtype(at::kFloat));
  dim3 grid((unsigned)(N / G8_BN), (unsigned)(M / G8_BM));
  auto stream = at::cuda::getCurrentCUDAStream();
#define L8_HEAD(LIVE_)                                                      \
  hipLaunchKernelGGL(                                                       \
      (gemm_nt_8phase_kernel<Epi::ReluDot, true, true, false, LIVE_>),      \
      grid, dim3(G8_THREADS), 0, stream, (const bf16_t*)x.data_ptr(),       \
      (const bf16_t*)w.data_ptr(), b2.data_ptr<float>(),                    \
      w3.data_ptr<float>(), nullptr, y.data_ptr(), M, N, K, n_live)
  if (n_live) L8_HEAD(true);
  else        L8_HEAD(false);
#undef L8_HEAD
  return y;
}

// ---- launcher (called from gemm.hip's dispatch) ---------------------------
void launch_gemm8(Epi epi, bool has_bias, bool out_fp32, bool emit_mask,
                  const void* ap, const void* bp, const float* bias,
                  const unsigned char* mask, unsigned char* mask_out,
                  void* cp, long long M, long long N, long long K) {
  dim3 grid((unsigned)((N + G8_BN - 1) / G8_BN),
            (unsigned)((M + G8_BM - 1) / G8_BM));
  auto stream = at::cuda::getCurrentCUDAStream();
  const bf16_t* a = (const bf16_t*)ap;
  const bf16_t* b = (const bf16_t*)bp;
#define L8(EPI_, HB_, OF_, EM_)                                             \
  hipLaunchKernelGGL((gemm_nt_8phase_kernel<EPI_, HB_, OF_, EM_>), grid,    \
                     dim3(G8_THREADS), 0, stream, a, b, bias, mask,         \
                     mask_out, cp, M, N, K)
  if (epi == Epi::BiasRelu && emit_mask) {
    if (has_bias) L8(Epi::BiasRelu, true, false, true);
    else          L8(Epi::BiasRelu, false, false, true);
  } else if (epi == Epi::BiasRelu) {
    if (has_bias) { if (out_fp32) L8(Epi::BiasRelu, true, true, false);
                    else          L8(Epi::BiasRelu, true, false, false); }
    else          { if (out_fp32) L8(Epi::BiasRelu, false, true, false);
                    else          L8(Epi::BiasRelu, false, false, false); }
  } else if (epi == Epi::MaskMul) {
    if (out_fp32) L8(Epi::MaskMul, false, true, false);
    else          L8(Epi::MaskMul, false, false, false);
  } else {
    if (out_fp32) L8(Epi::None, false, true, false);
    else          L8(Epi::None, false, false, false);
  }
#undef L8
}
