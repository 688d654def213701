// Fused OLS statistics, batched scoring and metric reductions — gfx950.
//
// Replaces sklearn LinearRegression.fit / predict and the sklearn metric
// calls (reference stage_1:79-108, stage_2:78, stage_4:101-113) with:
//   - linreg_stats:   single pass over (X, y) producing fp64
//                     [n, sum_x, sum_y, sum_xx, sum_xy] — the whole
//                     closed-form fit input AND the whole DP all-reduce
//                     payload.
//   - linear_score:   yhat = intercept + coef*X, float4-vectorised,
//                     grid-stride (hipGraph-capturable: no allocs/syncs).
//   - regression_metrics / score_label_metrics: one fused pass producing
//     every sum the MAPE/R^2/max-residual/Pearson formulas need.
//   - interval_coverage: how many rows fall inside up to four constant
//     prediction bands, as one more statistic of the same skeleton.
//   - linreg_split_stats / linear_split_metrics: the same two passes with
//     the philox train/test flag of random_split evaluated in-kernel, so
//     the linear fit never materialises the split.
//   - poly_stats / poly_fold_stats: the same for the polynomial ridge
//     family — the implicit-basis X^T X / X^T y of one degree, and the 18
//     power sums per cross-validation fold that carry the K-fold CV of
//     every degree <= 5 and every l2.
// All reductions are two-stage and atomic-free: per-wave shuffle -> LDS ->
// one plain store per block and statistic into a [grid, K] fp64 workspace,
// then a finalise kernel (one block, or one block per statistic where K is
// large) that combines the partials in a fixed order.  (One fp64 atomic
// per block and statistic into the same few addresses costs ~12 ns each on
// MI355X — 250 us for an 80 MB pass that streams in 19 us — and makes the
// sums depend on arrival order; the two-stage form is bitwise
// reproducible.)  Accumulation in fp64 so
// 1B-row sums stay exact to ~2^-40.  Stage 1 of the streaming reductions
// is one kernel (stream_reduce.h) instantiated over the statistic types
// below; two_stage_reduce is the one host driver.
#include <ATen/cuda/CUDAContext.h>
#include <hip/hip_runtime.h>
#include <torch/extension.h>

#include "host_checks.h"
#include "live_rows.h"
#include "philox.h"
#include "stream_reduce.h"

// Reduction grid cap: 4 blocks of 256 threads on each of the 256 CUs (16
// waves per CU keeps a streaming fp64 pass at bandwidth), and the finalise
// block then reads at most 1024 partials per statistic.
#define RED_GRID_CAP 1024
// elementwise (scoring) kernels: Guideline 11 cap
#define STREAM_GRID_CAP 2048

// blocks of RED_BLOCK threads for n rows at per_thread rows per thread and
// sweep, at most `cap` of them
static inline int capped_grid(long long n, int cap, int per_thread = 4) {
  long long want = (n + (long long)RED_BLOCK * per_thread - 1) /
                   ((long long)RED_BLOCK * per_thread);
  return (int)std::max<long long>(std::min<long long>(want, cap), 1);
}

// ---- stage 2 of every reduction ------------------------------------------
// ws is [nblocks, K]; statistic k is a max where bit k of max_mask is set,
// else a sum.  Writes out[off + k]; with off == 1 also out[0] = n.  One
// block, fixed combine order: thread t takes partials t, t+256, ...

__global__ void reduce_finalize_kernel(const double* __restrict__ ws,
                                       double* __restrict__ out, int nblocks,
                                       int K, unsigned int max_mask, int off,
                                       double n) {
  __shared__ double lds[RED_WAVES];
  for (int k = 0; k < K; ++k) {
    const bool is_max = (max_mask >> k) & 1u;
    double v = 0.0;
    for (int g = threadIdx.x; g < nblocks; g += RED_BLOCK) {
      double p = ws[(long long)g * K + k];
      v = is_max ? fmax(v, p) : v + p;
    }
    v = is_max ? block_max_f64<RED_WAVES>(v, lds)
               : block_sum_f64<RED_WAVES>(v, lds);
    if (threadIdx.x == 0) out[off + k] = v;
  }
  if (off == 1 && threadIdx.x == 0) out[0] = n;
}

// The wide finalise, for a K too large to walk in one block (the one-block
// kernel is latency-bound per statistic): block k owns statistic k and
// combines its partials exactly as reduce_finalize_kernel does, so the two
// give the same bits.  Sums only.
__global__ void reduce_finalize_wide_kernel(const double* __restrict__ ws,
                                            double* __restrict__ out,
                                            int nblocks, int K, int off,
                                            double n) {
  __shared__ double lds[RED_WAVES];
  const int k = blockIdx.x;
  double v = 0.0;
  for (int g = threadIdx.x; g < nblocks; g += RED_BLOCK)
    v += ws[(long long)g * K + k];
  v = block_sum_f64<RED_WAVES>(v, lds);
  if (threadIdx.x == 0) {
    out[off + k] = v;
    if (off == 1 && k == 0) out[0] = n;
  }
}

static void launch_finalize(const double* ws, double* out, int nblocks, int K,
                            unsigned int max_mask, int off, double n,
                            bool wide, hipStream_t stream) {
  if (wide) {
    TORCH_CHECK(max_mask == 0u, "the wide finalise combines sums only");
    hipLaunchKernelGGL(reduce_finalize_wide_kernel, dim3(K), dim3(RED_BLOCK),
                       0, stream, ws, out, nblocks, K, off, n);
  } else {
    hipLaunchKernelGGL(reduce_finalize_kernel, dim3(1), dim3(RED_BLOCK), 0,
                       stream, ws, out, nblocks, K, max_mask, off, n);
  }
}

// Both stages of a reduction over n rows on `like`'s device: grid ->
// workspace -> stage 1 -> finalise.  launch(grid, ws, stream) starts the
// stage-1 kernel, which fills ws[grid, K].  `wide` picks the
// block-per-statistic finalise.
template <class Launch>
static at::Tensor two_stage_reduce(const at::Tensor& like, long long n,
                                   int per_thread, int K,
                                   unsigned int max_mask, int off,
                                   Launch launch, bool wide = false) {
  const int grid = capped_grid(n, RED_GRID_CAP, per_thread);
  auto ws = at::empty({(long long)grid * K}, like.options().dtype(at::kDouble));
  auto stream = at::cuda::getCurrentCUDAStream();
  launch(grid, ws.data_ptr<double>(), stream);
  auto out = at::empty({off + K}, ws.options());
  launch_finalize(ws.data_ptr<double>(), out.data_ptr<double>(), grid, K,
                  max_mask, off, (double)n, wide, stream);
  return out;
}

// stream_reduce2_kernel<Stat> over the fp32 tensors (a, b); the workspace
// and result layout come from Stat
template <class Stat>
static at::Tensor stream_reduce2(const at::Tensor& a, const at::Tensor& b,
                                 const Stat& s) {
  using L = stat_layout<Stat>;
  const long long n = a.numel();
  return two_stage_reduce(
      a, n, 4, L::K, L::MAX_MASK, L::OFF,
      [&](int grid, double* ws, hipStream_t stream) {
        hipLaunchKernelGGL((stream_reduce2_kernel<Stat>), dim3(grid),
                           dim3(RED_BLOCK), 0, stream, a.data_ptr<float>(),
                           b.data_ptr<float>(), ws, n, s);
      });
}

// ---- linreg_stats ---------------------------------------------------------

// ws row = [n_train?, sum_x, sum_y, sum_xx, sum_xy] over rows (x, y).
// SPLIT: a TEST row of random_split is skipped and the row starts with the
// train-row count.
template <bool SPLIT>
struct LinregSums {
  static constexpr int NSUM = 4;
  static constexpr int MAX_POS = -1;
  static constexpr bool COUNTS = SPLIT;
  SplitKey key;

  __device__ void begin() {}
  __device__ __forceinline__ void row(long long i, float x, float y,
                                      double (&sum)[NSUM], double&,
                                      unsigned int& cnt) const {
    double xd = x, yd = y;
    if (SPLIT) {
      // a dropped row contributes exact zeros to every sum
      const bool train = !is_test_row(key, (unsigned long long)i);
      xd = train ? xd : 0.0;
      yd = train ? yd : 0.0;
      cnt += train;
    }
    sum[0] += xd;
    sum[1] += yd;
    sum[2] = fma(xd, xd, sum[2]);
    sum[3] = fma(xd, yd, sum[3]);
  }
};

static void check_xy(const at::Tensor& x, const at::Tensor& y) {
  TORCH_CHECK(x.is_cuda() && y.is_cuda() && x.numel() == y.numel());
  TORCH_CHECK(x.scalar_type() == at::kFloat && y.scalar_type() == at::kFloat);
}

at::Tensor linreg_stats_hip(const at::Tensor& x, const at::Tensor& y) {
  check_xy(x, y);
  return stream_reduce2(x, y, LinregSums<false>{});
}

// [n_train, sum_x, sum_y, sum_xx, sum_xy] over the TRAIN rows of
// random_split(x, y, test_frac, seed), without materialising the split.
at::Tensor linreg_split_stats_hip(const at::Tensor& x, const at::Tensor& y,
                                  double test_frac, int64_t seed) {
  check_xy(x, y);
  return stream_reduce2(x, y, LinregSums<true>{split_key(seed, test_frac)});
}

// ---- linear_score ---------------------------------------------------------

__global__ void linear_score_kernel(const float* __restrict__ x,
                                    float* __restrict__ out,
                                    const float* __restrict__ ab,
                                    long long n,
                                    const int64_t* __restrict__ n_live) {
  // coefficients read from device memory so a captured hipGraph picks up
  // redeployed models without recapture (serving hot-swap).  n_live, when
  // given, is the live row count (device int64[1], clamped to the buffer
  // size n): a captured replay over a padded bucket then touches only the
  // rows that exist.
  const float a = ab[0], b = ab[1];
  if (n_live != nullptr) n = live_count(n_live, n);
  const long long stride = (long long)gridDim.x * blockDim.x;
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long n4 = n >> 2;
  const float4* x4 = (const float4*)x;
  float4* o4 = (float4*)out;
  for (long long j = i; j < n4; j += stride) {
    float4 v = x4[j];
    o4[j] = {fmaf(b, v.x, a), fmaf(b, v.y, a), fmaf(b, v.z, a),
             fmaf(b, v.w, a)};
  }
  for (long long j = n4 * 4 + i; j < n; j += stride)
    out[j] = fmaf(b, x[j], a);
}

// n_dev (optional int64[1] device tensor): score only the first n_dev
// rows; the rest of the output is left unwritten.
at::Tensor linear_score_hip(const at::Tensor& x, const at::Tensor& ab,
                            const c10::optional<at::Tensor>& n_dev) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kFloat);
  TORCH_CHECK(ab.is_cuda() && ab.numel() == 2 &&
              ab.scalar_type() == at::kFloat);
  const int64_t* n_live = n_live_ptr(n_dev, x, "linear_score");
  long long n = x.numel();
  auto out = at::empty_like(x);
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(linear_score_kernel, dim3(capped_grid(n, STREAM_GRID_CAP)),
                     dim3(RED_BLOCK), 0, stream, x.data_ptr<float>(),
                     out.data_ptr<float>(), ab.data_ptr<float>(), n, n_live);
  return out;
}

// ---- polynomial ridge: fused X^T X / X^T y over an IMPLICIT basis --------
// The k-feature generalisation of linreg_stats promised by the SURVEY
// mapping table: sufficient statistics for ridge/OLS over the normalised
// polynomial basis phi_j(x) = t^j, t = (x - mu)/s, j = 0..NF-1.  The
// design matrix is never materialised — each thread expands its rows'
// basis on the fly and accumulates the upper-triangular X^T X plus X^T y
// in fp64, so the pass reads exactly the 8 bytes/row the linear fit
// reads regardless of degree.  Output layout:
//   out[0]                    = n
//   out[1 .. T]               = upper triangle of X^T X, row-major
//                               (T = NF*(NF+1)/2)
//   out[T+1 .. T+NF]          = X^T y
// Host side solves the (ridge-regularised) normal equations.

// Keeps a loop of its own (one row per thread, no float4, NF-dependent
// accumulator count); shares the per-block reduce-and-store and the host
// driver with the streaming reductions.
template <int NF>
__global__ void poly_stats_kernel(const float* __restrict__ x,
                                  const float* __restrict__ y,
                                  double* __restrict__ ws, long long n,
                                  float mu, float inv_s) {
  constexpr int TRI = NF * (NF + 1) / 2;
  double acc[TRI + NF];
#pragma unroll
  for (int i = 0; i < TRI + NF; ++i) acc[i] = 0.0;
  const long long stride = (long long)gridDim.x * RED_BLOCK;
  for (long long j = (long long)blockIdx.x * RED_BLOCK + threadIdx.x; j < n;
       j += stride) {
    double t = (double)((x[j] - mu) * inv_s);
    double yv = y[j];
    double phi[NF];
    phi[0] = 1.0;
#pragma unroll
    for (int p = 1; p < NF; ++p) phi[p] = phi[p - 1] * t;
    int s = 0;
#pragma unroll
    for (int a = 0; a < NF; ++a) {
#pragma unroll
      for (int b = a; b < NF; ++b) acc[s++] += phi[a] * phi[b];
    }
#pragma unroll
    for (int a = 0; a < NF; ++a) acc[TRI + a] += phi[a] * yv;
  }
  __shared__ double lds[RED_WAVES];
#pragma unroll
  for (int i = 0; i < TRI + NF; ++i)
    block_reduce_store<false>(
        acc[i], lds, ws, (long long)blockIdx.x * (TRI + NF) + i);
}

at::Tensor poly_stats_hip(const at::Tensor& x, const at::Tensor& y,
                          int64_t nf, double mu, double s) {
  check_xy(x, y);
  TORCH_CHECK(nf >= 2 && nf <= 6, "poly_stats: 2 <= degree+1 <= 6");
  const long long n = x.numel();
  const int K = (int)(nf * (nf + 1) / 2 + nf);
  const float inv_s = (float)(1.0 / s);
  // one row per thread and sweep here, so 1 per_thread
  return two_stage_reduce(
      x, n, 1, K, 0u, 1, [&](int grid, double* ws, hipStream_t stream) {
#define PS_LAUNCH(NF_)                                                      \
  hipLaunchKernelGGL((poly_stats_kernel<NF_>), dim3(grid), dim3(RED_BLOCK), \
                     0, stream, x.data_ptr<float>(), y.data_ptr<float>(),   \
                     ws, n, (float)mu, inv_s)
        switch (nf) {
          case 2: PS_LAUNCH(2); break;
          case 3: PS_LAUNCH(3); break;
          case 4: PS_LAUNCH(4); break;
          case 5: PS_LAUNCH(5); break;
          default: PS_LAUNCH(6); break;
        }
#undef PS_LAUNCH
      });
}

// ---- poly_fold_stats: K-fold statistics of every degree 1..5 in one pass --
// For the basis phi_j = t^j, PhiT Phi is the Hankel matrix of the power
// sums S_p = sum t^p, PhiT y is T_q = sum y t^q, and the squared error of
// any coefficient vector b on any row subset is Q - 2 bT T + bT H b with
// Q = sum y^2.  So per fold the PF_K = 18 sums
//   [S_0..S_10, T_0..T_5, Q]            (S_0 = the fold's row count)
// hold the complete K-fold cross-validation of every degree <= 5 and every
// l2: training statistics of fold f = total - fold f.  out is [F, PF_K].
// Row i belongs to fold_of_row(key, i, F) (philox.h).
#define PF_MAXDEG 5
#define PF_NS (2 * PF_MAXDEG + 1)          // S_0..S_10
#define PF_K (PF_NS + PF_MAXDEG + 1 + 1)   // + T_0..T_5 + Q

// Keeps a loop of its own like poly_stats_kernel.  acc[F * PF_K] lives in
// registers (F = 5: 180 of the 256 a 2-waves/SIMD kernel may hold, which
// is why F stops at 5); a row is folded into every fold's accumulators
// with a 0/1 weight, so there is no divergence and no indexed register
// access.  t and its powers round exactly as in poly_stats_kernel.
template <int F>
__global__ void __launch_bounds__(RED_BLOCK)
poly_fold_stats_kernel(const float* __restrict__ x,
                       const float* __restrict__ y, double* __restrict__ ws,
                       long long n, float mu, float inv_s, PhiloxKey key) {
  static_assert(RED_WAVES == 4, "the block tail below combines 4 waves");
  constexpr int K = F * PF_K;
  double acc[K];  // [F][PF_K]
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = 0.0;
  const long long stride = (long long)gridDim.x * RED_BLOCK;
  for (long long j = (long long)blockIdx.x * RED_BLOCK + threadIdx.x; j < n;
       j += stride) {
    const double t = (double)((x[j] - mu) * inv_s);
    const double yv = y[j];
    double v[PF_K];
    v[0] = 1.0;
#pragma unroll
    for (int p = 1; p < PF_NS; ++p) v[p] = v[p - 1] * t;
#pragma unroll
    for (int q = 0; q <= PF_MAXDEG; ++q) v[PF_NS + q] = yv * v[q];
    v[PF_K - 1] = yv * yv;
    const unsigned int fold = fold_of_row(key, (unsigned long long)j, F);
#pragma unroll
    for (int f = 0; f < F; ++f) {
      const double w = fold == (unsigned int)f ? 1.0 : 0.0;
#pragma unroll
      for (int k = 0; k < PF_K; ++k)
        acc[f * PF_K + k] = fma(w, v[k], acc[f * PF_K + k]);
    }
  }
  // block tail: all K statistics through one LDS array and ONE barrier
  // (block_reduce_store would take two per statistic, and a full shuffle
  // butterfly each).  wave_sum_scatter_f64 gives the bits of wave_sum_f64;
  // the four wave sums then combine as (w0 + w2) + (w1 + w3), which is
  // what block_sum_f64's xor butterfly computes.
  __shared__ double lds[RED_WAVES][K];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  wave_sum_scatter_f64<K>(acc, lane);
#pragma unroll
  for (int e = 0; e < wave_scatter_len<K>(); ++e) {
    const int k = wave_scatter_index<K>(e, lane);
    if (k >= 0) lds[wave][k] = acc[e];
  }
  __syncthreads();
  if (threadIdx.x < K) {
    const int k = threadIdx.x;
    ws[(long long)blockIdx.x * K + k] =
        (lds[0][k] + lds[2][k]) + (lds[1][k] + lds[3][k]);
  }
}

at::Tensor poly_fold_stats_hip(const at::Tensor& x, const at::Tensor& y,
                               int64_t folds, int64_t seed, double mu,
                               double s) {
  check_xy(x, y);
  TORCH_CHECK(folds >= 2 && folds <= 5, "poly_fold_stats: 2 <= folds <= 5");
  const long long n = x.numel();
  if (n == 0)
    return at::zeros({folds, PF_K}, x.options().dtype(at::kDouble));
  const float inv_s = (float)(1.0 / s);
  const PhiloxKey key = fold_key(seed);
  // one row per thread and sweep, as poly_stats
  return two_stage_reduce(
             x, n, 1, (int)folds * PF_K, 0u, 0,
             [&](int grid, double* ws, hipStream_t stream) {
#define PF_LAUNCH(F_)                                                     \
  hipLaunchKernelGGL((poly_fold_stats_kernel<F_>), dim3(grid),            \
                     dim3(RED_BLOCK), 0, stream, x.data_ptr<float>(),     \
                     y.data_ptr<float>(), ws, n, (float)mu, inv_s, key)
               switch (folds) {
                 case 2: PF_LAUNCH(2); break;
                 case 3: PF_LAUNCH(3); break;
                 case 4: PF_LAUNCH(4); break;
                 default: PF_LAUNCH(5); break;
               }
#undef PF_LAUNCH
             },
             /*wide=*/true)
      .view({folds, PF_K});
}

// Stage 2 alone over a [nblocks, K] fp64 workspace of sums, through the
// one-block or the wide finalise: the two give the same bits, which is
// what the tests and the A/B timing of the two kernels use this for.
at::Tensor reduce_finalize_hip(const at::Tensor& ws, bool wide) {
  TORCH_CHECK(ws.is_cuda() && ws.scalar_type() == at::kDouble &&
              ws.dim() == 2 && ws.is_contiguous() && ws.size(0) >= 1 &&
              ws.size(1) >= 1, "reduce_finalize: ws is a contiguous fp64 "
              "[nblocks, K] device tensor");
  auto out = at::empty({ws.size(1)}, ws.options());
  launch_finalize(ws.data_ptr<double>(), out.data_ptr<double>(),
                  (int)ws.size(0), (int)ws.size(1), 0u, 0, 0.0, wide,
                  at::cuda::getCurrentCUDAStream());
  return out;
}

// Horner-scheme polynomial scoring in the normalised basis; coefficients
// read from device memory so captured serving graphs follow redeploys.
__global__ void poly_score_kernel(const float* __restrict__ x,
                                  float* __restrict__ outv,
                                  const float* __restrict__ coef, int nf,
                                  float mu, float inv_s, long long n) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < n;
       j += stride) {
    float t = (x[j] - mu) * inv_s;
    float acc = coef[nf - 1];
    for (int p = nf - 2; p >= 0; --p) acc = fmaf(acc, t, coef[p]);
    outv[j] = acc;
  }
}

at::Tensor poly_score_hip(const at::Tensor& x, const at::Tensor& coef,
                          double mu, double s) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kFloat);
  TORCH_CHECK(coef.is_cuda() && coef.scalar_type() == at::kFloat &&
              coef.numel() >= 2);
  long long n = x.numel();
  auto out = at::empty_like(x);
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(poly_score_kernel, dim3(capped_grid(n, STREAM_GRID_CAP)),
                     dim3(RED_BLOCK), 0, stream, x.data_ptr<float>(),
                     out.data_ptr<float>(), coef.data_ptr<float>(),
                     (int)coef.numel(), (float)mu, (float)(1.0 / s), n);
  return out;
}

// ---- regression_metrics (offline: stage_1:79-90 semantics) ---------------
// out = [n, sum_ape, ss_res, sum_y, sum_yy, max_resid]
//
// ws row = [n_test?, sum_ape, ss_res, sum_y, sum_yy, max_resid] over rows
// (y, p).  Plain: p is the prediction.  SPLIT: p is the feature x, yhat =
// fmaf(b, x, a) is computed in fp32 exactly as linear_score_kernel does,
// only the TEST rows of random_split count, and the row starts with their
// count.
template <bool SPLIT>
struct RegressionSums {
  static constexpr int NSUM = 4;
  static constexpr int MAX_POS = 4;
  static constexpr bool COUNTS = SPLIT;
  const float* ab;  // SPLIT: device [intercept, coef]
  SplitKey key;
  float a, b;

  __device__ void begin() {
    if (SPLIT) { a = ab[0]; b = ab[1]; }
  }
  __device__ __forceinline__ void row(long long i, float yf, float pf,
                                      double (&sum)[NSUM], double& mx,
                                      unsigned int& cnt) const {
    const double MAPE_EPS = 2.220446049250313e-16;  // sklearn epsilon
    if (SPLIT) {
      // a non-test row becomes (y, yhat) = (0, 0): zero in every sum and
      // in the max
      const bool test = is_test_row(key, (unsigned long long)i);
      pf = test ? fmaf(b, pf, a) : 0.f;
      yf = test ? yf : 0.f;
      cnt += test;
    }
    double yv = yf, r = yv - pf;
    double ar = fabs(r);
    sum[0] += ar / fmax(fabs(yv), MAPE_EPS);
    sum[1] = fma(r, r, sum[1]);
    sum[2] += yv;
    sum[3] = fma(yv, yv, sum[3]);
    mx = fmax(mx, ar);
  }
};

at::Tensor regression_metrics_hip(const at::Tensor& y,
                                  const at::Tensor& yhat) {
  TORCH_CHECK(y.is_cuda() && yhat.is_cuda() && y.numel() == yhat.numel());
  auto yf = y.scalar_type() == at::kFloat ? y : y.to(at::kFloat);
  auto pf = yhat.scalar_type() == at::kFloat ? yhat : yhat.to(at::kFloat);
  return stream_reduce2(yf, pf, RegressionSums<false>{});
}

// [n_test, sum_ape, ss_res, sum_y, sum_yy, max_resid] of the linear model
// ab = [intercept, coef] over the TEST rows of random_split(x, y,
// test_frac, seed): split, predict and regression_metrics in one pass.
at::Tensor linear_split_metrics_hip(const at::Tensor& x, const at::Tensor& y,
                                    const at::Tensor& ab, double test_frac,
                                    int64_t seed) {
  check_xy(x, y);
  TORCH_CHECK(ab.is_cuda() && ab.numel() == 2 &&
              ab.scalar_type() == at::kFloat);
  return stream_reduce2(
      y, x,
      RegressionSums<true>{ab.data_ptr<float>(), split_key(seed, test_frac)});
}

// ---- score_label_metrics (online: stage_4:87-113 semantics) ---------------
// out = [n, sum_ape, max_ape, s_s, s_l, s_ss, s_ll, s_sl]
//
// ws row = [sum_ape, max_ape, s_s, s_l, s_ss, s_ll, s_sl] over rows
// (score, label) = out[1..7]
struct ScoreLabelSums {
  static constexpr int NSUM = 6;
  static constexpr int MAX_POS = 1;
  static constexpr bool COUNTS = false;

  __device__ void begin() {}
  __device__ __forceinline__ void row(long long, float s, float l,
                                      double (&sum)[NSUM], double& mx,
                                      unsigned int&) const {
    double sv = s, lv = l;
    double ape = fabs(sv / lv - 1.0);  // reference has no eps guard
    sum[0] += ape;
    mx = fmax(mx, ape);
    sum[1] += sv;
    sum[2] += lv;
    sum[3] = fma(sv, sv, sum[3]);
    sum[4] = fma(lv, lv, sum[4]);
    sum[5] = fma(sv, lv, sum[5]);
  }
};

at::Tensor score_label_metrics_hip(const at::Tensor& s, const at::Tensor& l) {
  TORCH_CHECK(s.is_cuda() && l.is_cuda() && s.numel() == l.numel());
  auto sf = s.scalar_type() == at::kFloat ? s : s.to(at::kFloat);
  auto lf = l.scalar_type() == at::kFloat ? l : l.to(at::kFloat);
  return stream_reduce2(sf, lf, ScoreLabelSums{});
}

// ---- interval_coverage (conformal bands: |label - score| <= half-width) ----
// out = [n, c0, c1, c2, c3]
//
// ws row = [c0..c3] over rows (score, label): c_q counts the rows with
// fabsf(__fsub_rn(label, score)) <= h[q], the residual of resid_select.h's
// key rule.  h is four fp32 half-widths in device memory; an unused level
// is passed as -1 and never counts, a NaN residual never counts, and +inf
// covers every other row.  The counts are exact integers in fp64.
struct CoverageSums {
  static constexpr int NSUM = 4;
  static constexpr int MAX_POS = -1;
  static constexpr bool COUNTS = false;
  const float* hw;  // device fp32[4]
  float h[NSUM];

  __device__ void begin() {
#pragma unroll
    for (int q = 0; q < NSUM; ++q) h[q] = hw[q];
  }
  __device__ __forceinline__ void row(long long, float s, float l,
                                      double (&sum)[NSUM], double&,
                                      unsigned int&) const {
    const float r = fabsf(__fsub_rn(l, s));
#pragma unroll
    for (int q = 0; q < NSUM; ++q) sum[q] += r <= h[q] ? 1.0 : 0.0;
  }
};

at::Tensor interval_coverage_hip(const at::Tensor& s, const at::Tensor& l,
                                 const at::Tensor& halfwidths) {
  TORCH_CHECK(s.is_cuda() && l.is_cuda() && s.numel() == l.numel());
  TORCH_CHECK(s.scalar_type() == at::kFloat && l.scalar_type() == at::kFloat &&
              s.is_contiguous() && l.is_contiguous());
  TORCH_CHECK(halfwidths.is_cuda() && halfwidths.scalar_type() == at::kFloat &&
                  halfwidths.is_contiguous() && halfwidths.numel() == 4,
              "interval_coverage: halfwidths is a float32[4] device tensor "
              "(unused levels -1)");
  return stream_reduce2(s, l, CoverageSums{halfwidths.data_ptr<float>()});
}
