// 256x256-tile 8-phase software-pipelined NT MFMA GEMM (gfx950).
//
// The deep-pipeline variant of gemm.hip's 128^2 kernel (which sits at
// the documented plain-HIP 2-phase ceiling, ~1000 TF): 16 waves per
// 1024-thread block (4x4), per-wave C = 64x64 = 4x4 fragments; one
// K-tile (BK=64) is four quadrants of 8 MFMAs, run as two phases of 16
// with the operand traffic software-pipelined at HALF-TILE (16 KiB)
// granularity.  Coordinates, live-row preamble, stager, prologue and the
// landing wait are tile256.h's; the schedule per tile T (slots T%2) is
//
//   phase A: wait vmcnt(2) [vmcnt(0) on the last tile]; barrier
//            issue A(T+1); read B(T) x8 + A q0,q1; MFMA q0+q1
//   phase B: barrier
//            issue B(T+2); read A q2,q3;            MFMA q2+q3
//
// Landing: the loop issues A(T+1) before B(T+2), which is all tile256.h's
// proof asks.  Slot safety is completion-airtight: A(T+1) overwrites
// A(T-1), whose q2/q3 reads were CONSUMED by MFMAs before any wave passed
// barrier(T,A); B(T+2) overwrites B(T), whose reads were consumed by MFMA
// q0/q1 before barrier(T,B).
// History: the first schedule had four phases of 8 MFMAs per tile and a
// vmcnt(4) wait; two phases halve the barriers.
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
#include "gemm_host.h"
#include "tile256.h"

#define G8_BK 64
#define G8_HT (128 * 64)  // shorts per half-tile slot

// The epilogue's read-only operand rides in ONE kernel-argument slot typed by
// the mode: w3 (fp32 [N]) for the fused scoring head, else the 1-bit mask.
template <Epi EPI>
using EpiOperand = std::conditional_t<EPI == Epi::ReluDot, const float*,
                                      const unsigned char*>;

// LIVE (the scoring head only): row tiles at or past the device-side live
// row count return at once and rows at or past it add nothing to y (same
// contract as gemm_mx8.hip's head).
template <Epi EPI, bool HAS_BIAS, bool OUT_FP32, bool EMIT_MASK = false,
          bool LIVE = false>
__launch_bounds__(T256_THREADS)
__global__ void gemm_nt_8phase_kernel(
    const bf16_t* __restrict__ A,  // [M,K]
    const bf16_t* __restrict__ B,  // [N,K]
    const float* __restrict__ bias, EpiOperand<EPI> __restrict__ epi_in,
    unsigned char* __restrict__ mask_out, void* __restrict__ C, long long M,
    long long N, long long K,
    const int64_t* __restrict__ n_live = nullptr) {  // LIVE only
  // ONE __shared__ object (guide §5 trap (a))
  __shared__ short lds[8 * G8_HT];  // [op A=0/B=1][buf][half][128][64]
  int live_rows;
  if (!tile256_live<EPI, LIVE>(n_live, M, live_rows)) return;
  const Tile256 tc = tile256_coords();
  const long long m0 = tc.m0, n0 = tc.n0;
  const int wm = tc.wm, wn = tc.wn, fl = tc.fl, kg = tc.kg;
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
  zero_acc(acc);

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

  // per-lane staging byte offset (tile-invariant): thread ci stages LDS
  // chunk ci&7 of row ci>>3, which holds source chunk (ci&7) ^ (row&7)
  int stg_off;
  {
    int ci = (int)threadIdx.x;
    int row = ci >> 3;
    int sc = (ci & 7) ^ (row & 7);
    stg_off = (int)((row * K + sc * 8) * 2);
  }
  const Tile256Src src = tile256_src(A, B, m0, n0, K);
#define G8_KOFF(T) ((long long)(T) * (G8_BK * 2))
#define G8_STAGE(slot, from) tile256_stage_half((char*)(slot), from, stg_off)

  tile256_prologue((char*)G8_ASLOT(0, 0), (char*)G8_BSLOT(0, 0),
                   (char*)G8_BSLOT(1, 0), src, stg_off, G8_KOFF(1), nt > 1);

  // Schedule and slot safety: see the file header.  Reads feed the SAME
  // phase's MFMAs (lgkm waits are in-phase).
#define G8_PHASE_A(T, TPAR)                                                 \
  do {                                                                      \
    tile256_wait_landed((T) + 1 < nt);                                      \
    __builtin_amdgcn_s_barrier();                                           \
    if ((T) + 1 < nt) {                                                     \
      G8_STAGE(G8_ASLOT(1 - (TPAR), 0), src.a0 + G8_KOFF((T) + 1));         \
      G8_STAGE(G8_ASLOT(1 - (TPAR), 1), src.a1 + G8_KOFF((T) + 1));         \
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
      G8_STAGE(G8_BSLOT(TPAR, 0), src.b0 + G8_KOFF((T) + 2));               \
      G8_STAGE(G8_BSLOT(TPAR, 1), src.b1 + G8_KOFF((T) + 2));               \
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
#undef G8_STAGE

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
  const char* op = "gemm8_relu_dot";
  // two K-tiles per loop trip
  static const GemmFormat bf16{at::kBFloat16, "bf16", 2, 1, 2 * G8_BK, 0};
  const GemmOperands g = gemm256_operands(op, bf16, x, w);
  const float* b2p = epi_vec_n(op, "b2", b2, g.N);
  const float* w3p = epi_vec_n(op, "w3", w3, g.N);
  TORCH_CHECK(b2p && w3p && b2.device() == x.device() &&
                  w3.device() == x.device(),
              op, ": b2 and w3 are required, on the operands' device");
  const int64_t* n_live = n_live_ptr(n_dev, x, op);
  auto y = at::zeros({g.M}, x.options().dtype(at::kFloat));
  if (g.empty()) return y;
  auto stream = at::cuda::getCurrentCUDAStream();
#define L8_HEAD(LIVE_)                                                      \
  hipLaunchKernelGGL(                                                       \
      (gemm_nt_8phase_kernel<Epi::ReluDot, true, true, false, LIVE_>),      \
      g.grid(), dim3(T256_THREADS), 0, stream, (const bf16_t*)g.a,          \
      (const bf16_t*)g.b, b2p, w3p, nullptr, y.data_ptr(), g.M, g.N, g.K,   \
      n_live)
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
  dim3 grid((unsigned)((N + T256_TILE - 1) / T256_TILE),
            (unsigned)((M + T256_TILE - 1) / T256_TILE));
  auto stream = at::cuda::getCurrentCUDAStream();
  const bf16_t* a = (const bf16_t*)ap;
  const bf16_t* b = (const bf16_t*)bp;
#define L8(EPI_, HB_, OF_, EM_)                                             \
  hipLaunchKernelGGL((gemm_nt_8phase_kernel<EPI_, HB_, OF_, EM_>), grid,    \
                     dim3(T256_THREADS), 0, stream, a, b, bias, mask,       \
                     mask_out, cp, M, N, K)
  if (epi == Epi::BiasRelu && emit_mask) {  // bf16 output only
    if (has_bias) L8(Epi::BiasRelu, true, false, true);
    else          L8(Epi::BiasRelu, false, false, true);
  } else if (epi == Epi::MaskMul) {
    if (out_fp32) L8(Epi::MaskMul, false, true, false);
    else          L8(Epi::MaskMul, false, false, false);
  } else {
    dispatch_epilogue(epi == Epi::BiasRelu, has_bias, out_fp32,
                      [&](auto e, auto hb, auto of) {
                        L8(decltype(e)::value, decltype(hb)::value,
                           decltype(of)::value, false);
                      });
  }
#undef L8
}
