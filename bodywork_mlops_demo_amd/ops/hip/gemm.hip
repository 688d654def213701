// Hand-written gfx950 MFMA bf16 dense GEMM — the MLP hot path.
//
// Replaces the sklearn/library matmuls of the reference's fit/predict
// (stage_1:105-106, stage_2:78) for the MLP config (BASELINE config 5)
// with v_mfma_f32_16x16x32_bf16 tiles, LDS-staged, fp32 accumulate.
//
// Two kernels, chosen so every global load is K-contiguous and every LDS
// fragment read is a single ds_read_b128 (CDNA4 fragment layout: a lane
// holds 8 contiguous K elements):
//   linear_nt:  C[M,N] = X[M,K] @ W[N,K]^T (+bias) (+ReLU | *mask) —
//               torch.nn.functional.linear convention; both operands
//               K-major so LDS staging is coalesced and linear.
//   gemm_tn:    C[M,N] = A[R,M]^T @ B[R,N] — the dW = dY^T @ X backward
//               shape; operands are R-major so tiles are transpose-staged
//               into the same K-contiguous LDS images.
//
// Geometry: 128x128 C-tile per 256-thread block (4 waves as 2x2, each
// wave a 64x64 sub-tile = 4x4 fragments of 16x16), BK=64.
// LDS layouts: the glds hot path uses lane-linear [128][64] tiles with a
// 16-B-chunk XOR swizzle carried on the SOURCE address and the fragment
// read (both-sides rule; PMC-measured 0 bank conflicts); the fallback
// register-staged kernels pad rows to 72 shorts (144-B stride) instead.
// fp32 C/D per guide §3: col = lane&15, row = (lane>>4)*4 + reg.
// The epilogue of a wave's 64x64 block (tile_epilogue, modes Epi::*) is
// shared with gemm8.hip and gemm_mx8.hip: mfma_tile.h.
#include <ATen/cuda/CUDAContext.h>
#include <hip/hip_runtime.h>
#include <torch/extension.h>

#include "bf16_utils.h"
#include "mfma_tile.h"

#define BM 128
#define BN 128
#define BK 64
#define LDS_STRIDE 72  // BK + 8 shorts pad
#define GEMM_THREADS 256

// stage a [ROWS x BK] K-major tile (row-major source, K contiguous):
// thread t loads 16 B chunks; zero-fill outside (r1, k1) bounds.
__device__ __forceinline__ void stage_k_major(
    short* __restrict__ lds, const bf16_t* __restrict__ src, long long ld,
    long long row0, long long row_end, long long k0, long long k_end) {
#pragma unroll
  for (int it = 0; it < (BM * (BK / 8)) / GEMM_THREADS; ++it) {
    int chunk = threadIdx.x + it * GEMM_THREADS;
    int r = chunk >> 3;          // row within tile
    int c8 = chunk & 7;          // 8-col chunk within BK
    long long gr = row0 + r;
    long long gk = k0 + c8 * 8;
    lds_vec val;
    if (gr < row_end && gk + 7 < k_end) {
      val = *(const lds_vec*)(src + gr * ld + gk);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        long long kk = gk + e;
        val.s[e] = (gr < row_end && kk < k_end)
                       ? ((const short*)(src + gr * ld))[kk]
                       : (short)0;
      }
    }
    *(lds_vec*)(lds + r * LDS_STRIDE + c8 * 8) = val;
  }
}

// stage a [ROWS x BK] K-major LDS tile from an R-major source
// (src[R, C] with R the GEMM K dim): transpose during the LDS write.
__device__ __forceinline__ void stage_transposed(
    short* __restrict__ lds, const bf16_t* __restrict__ src, long long ld,
    long long col0, long long col_end /* tile rows = source cols */,
    long long k0, long long k_end /* tile cols = source rows */) {
#pragma unroll
  for (int it = 0; it < (BM * (BK / 8)) / GEMM_THREADS; ++it) {
    int chunk = threadIdx.x + it * GEMM_THREADS;
    int kr = chunk >> 4;         // source row (= tile k) [0,64)
    int c8 = chunk & 15;         // 8-col chunk along source cols [0,16)
    long long gk = k0 + kr;
    long long gc = col0 + c8 * 8;
    lds_vec val;
    if (gk < k_end && gc + 7 < col_end) {
      val = *(const lds_vec*)(src + gk * ld + gc);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        long long cc = gc + e;
        val.s[e] = (gk < k_end && cc < col_end)
                       ? ((const short*)(src + gk * ld))[cc]
                       : (short)0;
      }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e)
      lds[(c8 * 8 + e) * LDS_STRIDE + kr] = val.s[e];
  }
}

// ---- glds-staged NT kernel (the hot path) --------------------------------
// global_load_lds dwordx4 staging straight into a lane-linear LDS image;
// the bank-conflict XOR swizzle lives on the SOURCE address and the
// fragment-read address (both-sides rule): LDS chunk (row, c) holds the
// logical 16-B chunk (row, c ^ (row & 7)).  Two LDS buffers, one
// vmcnt(0)+barrier per K-tile (the guide's "step 3" structure).

// stage a [128 x 64] bf16 tile: 16 wave-level 1-KiB glds per tile
__device__ __forceinline__ void stage_tile_glds(
    short* __restrict__ lds_tile, const bf16_t* __restrict__ src,
    long long ld, long long row0, long long row_max, long long k0) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    int ci0 = (p * 4 + wave) * 64;
    int ci = ci0 + lane;
    int row = ci >> 3;
    int sc = (ci & 7) ^ (row & 7);  // inverse source swizzle
    long long gr = row0 + row;
    if (gr >= row_max) gr = row_max - 1;  // clamp: junk rows masked later
    glds16(src + gr * ld + k0 + sc * 8, (char*)lds_tile + ci0 * 16);
  }
}

template <Epi EPI, bool HAS_BIAS, bool OUT_FP32, bool EMIT_MASK = false>
__launch_bounds__(GEMM_THREADS)
__global__ void gemm_nt_glds_kernel(
    const bf16_t* __restrict__ A,  // [M,K]
    const bf16_t* __restrict__ B,  // [N,K]
    const float* __restrict__ bias, const unsigned char* __restrict__ mask,
    unsigned char* __restrict__ mask_out,
    void* __restrict__ C, long long M, long long N, long long K) {
  __shared__ short lds_all[2 * 2 * 128 * 64];  // [buf][A/B][128][64]
  const long long m0 = (long long)blockIdx.y * BM;
  const long long n0 = (long long)blockIdx.x * BN;
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int wm = wave >> 1, wn = wave & 1;
  const int fl = lane & 15;
  const int kg = lane >> 4;
  const int swz = fl & 7;  // read-side XOR factor (row & 7 == fl & 7)

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  const int TILE = 128 * 64;  // shorts per tile

  stage_tile_glds(lds_all, A, K, m0, M, 0);
  stage_tile_glds(lds_all + 2 * TILE, B, K, n0, N, 0);

  __syncthreads();  // carries the vmcnt(0) for the in-flight glds

  // 2-phase loop, ONE barrier per K-tile: stage tile t+1 (other buffer)
  // before computing tile t; the __syncthreads at the tile end both
  // drains the glds (vmcnt(0)) and is the rendezvous, so tile t+1's data
  // is visible to every wave when the next iteration reads it.  A
  // counted-vmcnt raw-barrier variant was measured SLOWER here (it needs
  // two barriers per tile: wait-rendezvous + buffer-reuse; 762 vs 944 TF
  // at 4096^3) — the single merged barrier wins at this occupancy
  // (2 blocks/CU hides the drain).
  int cur = 0;
  for (long long k0 = 0; k0 < K; k0 += BK) {
    short* as_cur = lds_all + cur * TILE;
    short* bs_cur = lds_all + 2 * TILE + cur * TILE;
    if (k0 + BK < K) {
      stage_tile_glds(lds_all + (cur ^ 1) * TILE, A, K, m0, M, k0 + BK);
      stage_tile_glds(lds_all + 2 * TILE + (cur ^ 1) * TILE, B, K, n0, N,
                      k0 + BK);
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8_v a_frag[4], b_frag[4];
      const int cidx = ((ks * 4 + kg) ^ swz) * 8;
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        a_frag[f] =
            ((const lds_vec*)(as_cur + (wm * 64 + f * 16 + fl) * 64 + cidx))
                ->v;
        b_frag[f] =
            ((const lds_vec*)(bs_cur + (wn * 64 + f * 16 + fl) * 64 + cidx))
                ->v;
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a_frag[i], b_frag[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();  // drains next tile's glds; makes buffers reusable
    cur ^= 1;
  }
  tile_epilogue<EPI, HAS_BIAS, OUT_FP32, EMIT_MASK>(
      acc, bias, nullptr, mask, mask_out, C, M, N, m0, n0, wm, wn, fl, kg);
}

template <bool TN, Epi EPI, bool HAS_BIAS, bool OUT_FP32>
__launch_bounds__(GEMM_THREADS)
__global__ void gemm_bf16_kernel(
    const bf16_t* __restrict__ A,  // NT: [M,K]; TN: [R=K, M]
    const bf16_t* __restrict__ B,  // NT: [N,K]; TN: [R=K, N]
    const float* __restrict__ bias, const unsigned char* __restrict__ mask,
    void* __restrict__ C, long long M, long long N, long long K) {
  __shared__ short lds_all[2 * BM * LDS_STRIDE];
  short* As = lds_all;
  short* Bs = lds_all + BM * LDS_STRIDE;

  const long long m0 = (long long)blockIdx.y * BM;
  const long long n0 = (long long)blockIdx.x * BN;
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int wm = wave >> 1;  // wave row 0..1
  const int wn = wave & 1;   // wave col 0..1
  const int fl = lane & 15;       // fragment row/col within 16
  const int kg = lane >> 4;       // k-group 0..3 (8 elems each)

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  for (long long k0 = 0; k0 < K; k0 += BK) {
    if (TN) {
      stage_transposed(As, A, M, m0, M, k0, K);
      stage_transposed(Bs, B, N, n0, N, k0, K);
    } else {
      stage_k_major(As, A, K, m0, M, k0, K);
      stage_k_major(Bs, B, K, n0, N, k0, K);
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < BK / 32; ++ks) {
      bf16x8_v a_frag[4], b_frag[4];
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        a_frag[f] = ((const lds_vec*)(As + (wm * 64 + f * 16 + fl) * LDS_STRIDE +
                                      ks * 32 + kg * 8))->v;
        b_frag[f] = ((const lds_vec*)(Bs + (wn * 64 + f * 16 + fl) * LDS_STRIDE +
                                      ks * 32 + kg * 8))->v;
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a_frag[i], b_frag[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  }

  tile_epilogue<EPI, HAS_BIAS, OUT_FP32>(acc, bias, nullptr, mask, nullptr, C,
                                         M, N, m0, n0, wm, wn, fl, kg);
}

// ---- launchers ------------------------------------------------------------

static void launch_gemm(bool tn, Epi epi, bool has_bias, bool out_fp32,
                        const at::Tensor& a, const at::Tensor& b,
                        const float* bias, const unsigned char* mask,
                        unsigned char* mask_out, at::Tensor& c,
                        long long M, long long N, long long K) {
  dim3 grid((N + BN - 1) / BN, (M + BM - 1) / BM);
  auto stream = at::cuda::getCurrentCUDAStream();
  const bf16_t* ap = (const bf16_t*)a.data_ptr();
  const bf16_t* bp = (const bf16_t*)b.data_ptr();
  void* cp = c.data_ptr();

  // deep-pipeline 16-wave 256^2 8-phase kernel (gemm8.hip) for
  // exact-tile shapes — DEFAULT ON: A/B-measured on MI355X at
  // 1249-1292 TF vs this file's 128^2 kernel's 1011-1084 on the hot
  // shapes (profiles/r01_gemm_variant_study.md; +25% on the MLP
  // training cycle).  BODYWORK_GEMM_8PHASE=0 opts out.
  if (!tn && K % 128 == 0 && K >= 256 && K <= (1 << 22) && M % 256 == 0 &&
      N % 256 == 0 && M >= 256) {
    static int use8 = [] {
      const char* e = getenv("BODYWORK_GEMM_8PHASE");
      return (e && e[0] == '0') ? 0 : 1;
    }();
    if (use8) {
      launch_gemm8(epi, has_bias, out_fp32, mask_out != nullptr, ap, bp,
                   bias, mask, mask_out, cp, M, N, K);
      return;
    }
  }

  // hot path: NT with K a tile multiple -> glds-staged kernel
  if (!tn && K % BK == 0 && K > 0) {
    // (mask_out is read only by the EMIT_MASK instantiations)
#define G_GLDS(EPI_, HB_, OF_, EM_)                                         \
  hipLaunchKernelGGL((gemm_nt_glds_kernel<EPI_, HB_, OF_, EM_>), grid,      \
                     dim3(GEMM_THREADS), 0, stream, ap, bp, bias, mask,     \
                     mask_out, cp, M, N, K)
    if (epi == Epi::BiasRelu && mask_out != nullptr) {
      if (has_bias) { if (out_fp32) G_GLDS(Epi::BiasRelu, true, true, true);
                      else          G_GLDS(Epi::BiasRelu, true, false, true); }
      else          { if (out_fp32) G_GLDS(Epi::BiasRelu, false, true, true);
                      else          G_GLDS(Epi::BiasRelu, false, false, true); }
    } else if (epi == Epi::BiasRelu) {
      if (has_bias) { if (out_fp32) G_GLDS(Epi::BiasRelu, true, true, false);
                      else          G_GLDS(Epi::BiasRelu, true, false, false); }
      else          { if (out_fp32) G_GLDS(Epi::BiasRelu, false, true, false);
                      else          G_GLDS(Epi::BiasRelu, false, false, false); }
    } else if (epi == Epi::MaskMul) {
      if (out_fp32) G_GLDS(Epi::MaskMul, false, true, false);
      else          G_GLDS(Epi::MaskMul, false, false, false);
    } else {
      if (out_fp32) G_GLDS(Epi::None, false, true, false);
      else          G_GLDS(Epi::None, false, false, false);
    }
#undef G_GLDS
    return;
  }

#define G_LAUNCH(TN_, EPI_, HB_, OF_)                                       \
  hipLaunchKernelGGL((gemm_bf16_kernel<TN_, EPI_, HB_, OF_>), grid,         \
                     dim3(GEMM_THREADS), 0, stream, ap, bp, bias, mask, cp, \
                     M, N, K)
  /* mask_out unsupported on the fallback kernel (checked in hosts) */
#define G_EPI(TN_)                                                          \
  do {                                                                      \
    if (epi == Epi::BiasRelu) {                                             \
      if (has_bias) { if (out_fp32) G_LAUNCH(TN_, Epi::BiasRelu, true, true);  \
                      else          G_LAUNCH(TN_, Epi::BiasRelu, true, false); }\
      else          { if (out_fp32) G_LAUNCH(TN_, Epi::BiasRelu, false, true); \
                      else          G_LAUNCH(TN_, Epi::BiasRelu, false, false);}\
    } else if (epi == Epi::MaskMul) {                                       \
      if (out_fp32) G_LAUNCH(TN_, Epi::MaskMul, false, true);               \
      else          G_LAUNCH(TN_, Epi::MaskMul, false, false);              \
    } else {                                                                \
      if (out_fp32) G_LAUNCH(TN_, Epi::None, false, true);                  \
      else          G_LAUNCH(TN_, Epi::None, false, false);                 \
    }                                                                       \
  } while (0)
  if (tn) G_EPI(true); else G_EPI(false);
#undef G_EPI
#undef G_LAUNCH
}

// C = x @ w^T (+bias)(+relu | *mask); x [M,K], w [N,K]
at::Tensor linear_bf16_hip(const at::Tensor& x, const at::Tensor& w,
                           const c10::optional<at::Tensor>& bias, bool relu,
                           const c10::optional<at::Tensor>& mask,
                           bool out_fp32) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 && w.dim() == 2);
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 &&
              w.scalar_type() == at::kBFloat16);
  long long M = x.size(0), K = x.size(1), N = w.size(0);
  TORCH_CHECK(w.size(1) == K, "linear_bf16: w must be [N,K]");
  TORCH_CHECK(!(relu && mask.has_value()), "relu and mask are exclusive");
  auto c = at::empty({M, N},
                     x.options().dtype(out_fp32 ? at::kFloat : at::kBFloat16));
  at::Tensor bias_f;
  const float* bp = nullptr;
  if (bias.has_value()) {
    bias_f = bias->to(at::kFloat);
    bp = bias_f.data_ptr<float>();
  }
  Epi epi = mask.has_value() ? Epi::MaskMul
            : (relu || bias.has_value()) ? Epi::BiasRelu
                                         : Epi::None;
  // bias without relu: fold via Epi::BiasRelu only when relu requested;
  // else add bias in the same kernel without clamping -> use NONE + host
  // add would cost a pass, so clamp-free bias is handled here:
  TORCH_CHECK(!(bias.has_value() && !relu),
              "linear_bf16: bias currently requires relu epilogue");
  const unsigned char* mp = nullptr;
  if (mask.has_value()) {
    TORCH_CHECK(mask->scalar_type() == at::kByte &&
                    mask->numel() == M * (N / 8) && N % 8 == 0,
                "linear_bf16: mask must be a uint8 [M, N/8] relu bitmask");
    mp = (const unsigned char*)mask->data_ptr();
  }
  launch_gemm(false, epi, bias.has_value(), out_fp32, x, w, bp, mp, nullptr,
              c, M, N, K);
  return c;
}

// C, maskbits = relu(x @ w^T + bias): the forward hot path also emitting
// the 1-bit relu mask the backward consumes (uint8 [M, N/8]).
std::tuple<at::Tensor, at::Tensor> linear_relu_mask_bf16_hip(
    const at::Tensor& x, const at::Tensor& w,
    const c10::optional<at::Tensor>& bias) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 && w.dim() == 2);
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 &&
              w.scalar_type() == at::kBFloat16);
  long long M = x.size(0), K = x.size(1), N = w.size(0);
  TORCH_CHECK(w.size(1) == K && N % 16 == 0 && K % BK == 0,
              "linear_relu_mask: w [N,K], N%16==0, K%64==0");
  auto c = at::empty({M, N}, x.options());
  auto mask_out = at::empty({M, N / 8}, x.options().dtype(at::kByte));
  at::Tensor bias_f;
  const float* bp = nullptr;
  if (bias.has_value()) {
    bias_f = bias->to(at::kFloat);
    bp = bias_f.data_ptr<float>();
  }
  launch_gemm(false, Epi::BiasRelu, bias.has_value(), false, x, w, bp,
              nullptr, (unsigned char*)mask_out.data_ptr(), c, M, N, K);
  return {c, mask_out};
}

// C = a^T @ b; a [R,M], b [R,N] (the dW backward shape)
at::Tensor gemm_tn_bf16_hip(const at::Tensor& a, const at::Tensor& b,
                            bool out_fp32) {
  TORCH_CHECK(a.is_cuda() && a.dim() == 2 && b.dim() == 2);
  TORCH_CHECK(a.scalar_type() == at::kBFloat16 &&
              b.scalar_type() == at::kBFloat16);
  long long R = a.size(0), M = a.size(1), N = b.size(1);
  TORCH_CHECK(b.size(0) == R, "gemm_tn: row counts must match");
  auto c = at::empty({M, N},
                     a.options().dtype(out_fp32 ? at::kFloat : at::kBFloat16));
  launch_gemm(true, Epi::None, false, out_fp32, a, b, nullptr, nullptr,
              nullptr, c, M, N, R);
  return c;
}
