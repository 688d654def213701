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
//   - linreg_split_stats / linear_split_metrics: the same two passes with
//     the philox train/test flag of random_split evaluated in-kernel, so
//     the linear fit never materialises the split.
// All reductions are two-stage and atomic-free: per-wave shuffle -> LDS ->
// one plain store per block and statistic into a [grid, K] fp64 workspace,
// then a one-block finalise kernel that combines the partials in a fixed
// order.  (One fp64 atomic per block and statistic into the same few
// addresses costs ~12 ns each on MI355X — 250 us for an 80 MB pass that
// streams in 19 us — and makes the sums depend on arrival order; the
// two-stage form is bitwise reproducible.)  Accumulation in fp64 so
// 1B-row sums stay exact to ~2^-40.
#include <ATen/cuda/CUDAContext.h>
#include <hip/hip_runtime.h>
#include <torch/extension.h>

#include "host_checks.h"
#include "live_rows.h"
#include "philox.h"
#include "reduce.h"

#define RED_BLOCK 256
#define RED_WAVES (RED_BLOCK / 64)
// Reduction grid cap: 4 blocks of 256 threads on each of the 256 CUs (16
// waves per CU keeps a streaming fp64 pass at bandwidth), and the finalise
// block then reads at most 1024 partials per statistic.
#define RED_GRID_CAP 1024

// elementwise (scoring) kernels: Guideline 11 cap
static inline int stream_grid(long long n, int per_thread = 4) {
  long long want = (n + (long long)RED_BLOCK * per_thread - 1) /
                   ((long long)RED_BLOCK * per_thread);
  return (int)std::max<long long>(std::min<long long>(want, 2048), 1);
}

static inline int reduce_grid(long long n, int per_thread = 4) {
  long long want = (n + (long long)RED_BLOCK * per_thread - 1) /
                   ((long long)RED_BLOCK * per_thread);
  return (int)std::max<long long>(std::min<long long>(want, RED_GRID_CAP), 1);
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

static at::Tensor reduce_finalize(const at::Tensor& ws, int grid, int K,
                                  unsigned int max_mask, int off, double n,
                                  hipStream_t stream) {
  auto out = at::empty({off + K}, ws.options());
  hipLaunchKernelGGL(reduce_finalize_kernel, dim3(1), dim3(RED_BLOCK), 0,
                     stream, ws.data_ptr<double>(), out.data_ptr<double>(),
                     grid, K, max_mask, off, n);
  return out;
}

static inline void split_keys(int64_t seed, double test_frac,
                              unsigned int* key0, unsigned int* key1,
                              unsigned int* tau) {
  // must stay identical to random_split_hip (datagen.hip): same row sets
  *key0 = (unsigned int)(seed & 0xFFFFFFFFll);
  *key1 = (seed > 0xFFFFFFFFll) ? (unsigned int)(seed >> 32) : 0x85EBCA6Bu;
  *tau = (unsigned int)(test_frac * 4294967296.0);
}

// ---- linreg_stats ---------------------------------------------------------

// SPLIT: row i is skipped when it is a TEST row of random_split
// (philox(key, i).x < tau); ws then carries the train-row count as
// statistic 0, so K = 5 instead of 4.
template <bool SPLIT>
__global__ void linreg_stats_kernel(const float* __restrict__ x,
                                    const float* __restrict__ y,
                                    double* __restrict__ ws, long long n,
                                    unsigned int key0, unsigned int key1,
                                    unsigned int tau) {
  // 4 independent partial accumulators per statistic (one per float4
  // lane) break the per-iteration fp64 dependency chains that left the
  // serial version at ~12% of HBM bandwidth
  double sx[4] = {0, 0, 0, 0}, sy[4] = {0, 0, 0, 0};
  double sxx[4] = {0, 0, 0, 0}, sxy[4] = {0, 0, 0, 0};
  unsigned int cnt = 0;  // per-thread rows < 2^32
  const long long stride = (long long)gridDim.x * RED_BLOCK;
  long long i = (long long)blockIdx.x * RED_BLOCK + threadIdx.x;
  const long long n4 = n & ~3ll;
  for (long long j = i * 4; j < n4; j += stride * 4) {
    float4 xv = *(const float4*)(x + j);
    float4 yv = *(const float4*)(y + j);
    const float xs[4] = {xv.x, xv.y, xv.z, xv.w};
    const float ys[4] = {yv.x, yv.y, yv.z, yv.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      double xd = xs[e], yd = ys[e];
      if (SPLIT) {
        // a dropped row contributes exact zeros to every sum
        const bool train =
            philox4x32((unsigned long long)(j + e), key0, key1).x >= tau;
        xd = train ? xd : 0.0;
        yd = train ? yd : 0.0;
        cnt += train;
      }
      sx[e] += xd;
      sy[e] += yd;
      sxx[e] = fma(xd, xd, sxx[e]);
      sxy[e] = fma(xd, yd, sxy[e]);
    }
  }
  for (long long j = n4 + i; j < n; j += stride) {
    double xv = x[j], yv = y[j];
    if (SPLIT) {
      const bool train =
          philox4x32((unsigned long long)j, key0, key1).x >= tau;
      xv = train ? xv : 0.0;
      yv = train ? yv : 0.0;
      cnt += train;
    }
    sx[0] += xv; sy[0] += yv;
    sxx[0] = fma(xv, xv, sxx[0]);
    sxy[0] = fma(xv, yv, sxy[0]);
  }
#pragma unroll
  for (int e = 1; e < 4; ++e) {
    sx[0] += sx[e]; sy[0] += sy[e]; sxx[0] += sxx[e]; sxy[0] += sxy[e];
  }
  constexpr int K = SPLIT ? 5 : 4;
  double* row = ws + (long long)blockIdx.x * K;
  __shared__ double lds[RED_WAVES];
  double t;
  if (SPLIT) {
    t = block_sum_f64<RED_WAVES>((double)cnt, lds);
    if (threadIdx.x == 0) *row++ = t;
  }
  t = block_sum_f64<RED_WAVES>(sx[0], lds);
  if (threadIdx.x == 0) row[0] = t;
  t = block_sum_f64<RED_WAVES>(sy[0], lds);
  if (threadIdx.x == 0) row[1] = t;
  t = block_sum_f64<RED_WAVES>(sxx[0], lds);
  if (threadIdx.x == 0) row[2] = t;
  t = block_sum_f64<RED_WAVES>(sxy[0], lds);
  if (threadIdx.x == 0) row[3] = t;
}

at::Tensor linreg_stats_hip(const at::Tensor& x, const at::Tensor& y) {
  TORCH_CHECK(x.is_cuda() && y.is_cuda() && x.numel() == y.numel());
  TORCH_CHECK(x.scalar_type() == at::kFloat && y.scalar_type() == at::kFloat);
  long long n = x.numel();
  const int grid = reduce_grid(n);
  auto ws = at::empty({(long long)grid * 4}, x.options().dtype(at::kDouble));
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL((linreg_stats_kernel<false>), dim3(grid),
                     dim3(RED_BLOCK), 0, stream, x.data_ptr<float>(),
                     y.data_ptr<float>(), ws.data_ptr<double>(), n, 0u, 0u,
                     0u);
  return reduce_finalize(ws, grid, 4, 0u, 1, (double)n, stream);
}

// [n_train, sum_x, sum_y, sum_xx, sum_xy] over the TRAIN rows of
// random_split(x, y, test_frac, seed), without materialising the split.
at::Tensor linreg_split_stats_hip(const at::Tensor& x, const at::Tensor& y,
                                  double test_frac, int64_t seed) {
  TORCH_CHECK(x.is_cuda() && y.is_cuda() && x.numel() == y.numel());
  TORCH_CHECK(x.scalar_type() == at::kFloat && y.scalar_type() == at::kFloat);
  long long n = x.numel();
  unsigned int key0, key1, tau;
  split_keys(seed, test_frac, &key0, &key1, &tau);
  const int grid = reduce_grid(n);
  auto ws = at::empty({(long long)grid * 5}, x.options().dtype(at::kDouble));
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL((linreg_stats_kernel<true>), dim3(grid),
                     dim3(RED_BLOCK), 0, stream, x.data_ptr<float>(),
                     y.data_ptr<float>(), ws.data_ptr<double>(), n, key0,
                     key1, tau);
  return reduce_finalize(ws, grid, 5, 0u, 0, 0.0, stream);
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
  hipLaunchKernelGGL(linear_score_kernel, dim3(stream_grid(n)),
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
  for (int i = 0; i < TRI + NF; ++i) {
    double v = block_sum_f64<RED_WAVES>(acc[i], lds);
    if (threadIdx.x == 0) ws[(long long)blockIdx.x * (TRI + NF) + i] = v;
  }
}

at::Tensor poly_stats_hip(const at::Tensor& x, const at::Tensor& y,
                          int64_t nf, double mu, double s) {
  TORCH_CHECK(x.is_cuda() && y.is_cuda() && x.numel() == y.numel());
  TORCH_CHECK(x.scalar_type() == at::kFloat && y.scalar_type() == at::kFloat);
  TORCH_CHECK(nf >= 2 && nf <= 6, "poly_stats: 2 <= degree+1 <= 6");
  long long n = x.numel();
  int tri = (int)(nf * (nf + 1) / 2);
  const int K = tri + (int)nf;
  // one row per thread and sweep here, so 1 per_thread
  const int nblk = reduce_grid(n, 1);
  auto ws = at::empty({(long long)nblk * K}, x.options().dtype(at::kDouble));
  auto stream = at::cuda::getCurrentCUDAStream();
  dim3 grid(nblk);
  float inv_s = (float)(1.0 / s);
#define PS_LAUNCH(NF_)                                                     \
  hipLaunchKernelGGL((poly_stats_kernel<NF_>), grid, dim3(RED_BLOCK), 0,   \
                     stream, x.data_ptr<float>(), y.data_ptr<float>(),     \
                     ws.data_ptr<double>(), n, (float)mu, inv_s)
  switch (nf) {
    case 2: PS_LAUNCH(2); break;
    case 3: PS_LAUNCH(3); break;
    case 4: PS_LAUNCH(4); break;
    case 5: PS_LAUNCH(5); break;
    default: PS_LAUNCH(6); break;
  }
#undef PS_LAUNCH
  return reduce_finalize(ws, nblk, K, 0u, 1, (double)n, stream);
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
  hipLaunchKernelGGL(poly_score_kernel, dim3(stream_grid(n)),
                     dim3(RED_BLOCK), 0, stream, x.data_ptr<float>(),
                     out.data_ptr<float>(), coef.data_ptr<float>(),
                     (int)coef.numel(), (float)mu, (float)(1.0 / s), n);
  return out;
}

// ---- regression_metrics (offline: stage_1:79-90 semantics) ---------------
// out = [n, sum_ape, ss_res, sum_y, sum_yy, max_resid]
//
// SPLIT: `x` holds the feature, yhat = fmaf(b, x, a) is computed in fp32
// exactly as linear_score_kernel does, and only the TEST rows of
// random_split count (philox(key, i).x < tau); ws then carries the
// test-row count as statistic 0, so K = 6 instead of 5.

template <bool SPLIT>
__global__ void regression_metrics_kernel(const float* __restrict__ y,
                                          const float* __restrict__ x,
                                          const float* __restrict__ ab,
                                          double* __restrict__ ws,
                                          long long n, unsigned int key0,
                                          unsigned int key1,
                                          unsigned int tau) {
  const double MAPE_EPS = 2.220446049250313e-16;  // sklearn epsilon
  double s_ape[4] = {0, 0, 0, 0}, ss_res[4] = {0, 0, 0, 0};
  double s_y[4] = {0, 0, 0, 0}, s_yy[4] = {0, 0, 0, 0};
  double max_res = 0;
  unsigned int cnt = 0;
  float a = 0.f, b = 0.f;
  if (SPLIT) { a = ab[0]; b = ab[1]; }
  const long long stride = (long long)gridDim.x * RED_BLOCK;
  const long long i = (long long)blockIdx.x * RED_BLOCK + threadIdx.x;
  const long long n4 = n & ~3ll;
  for (long long j = i * 4; j < n4; j += stride * 4) {
    float4 yv4 = *(const float4*)(y + j);
    float4 pv4 = *(const float4*)(x + j);
    const float ys[4] = {yv4.x, yv4.y, yv4.z, yv4.w};
    const float ps[4] = {pv4.x, pv4.y, pv4.z, pv4.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float yf = ys[e], pf = ps[e];
      if (SPLIT) {
        // a non-test row becomes (y, yhat) = (0, 0): zero in every sum
        // and in the max
        const bool test =
            philox4x32((unsigned long long)(j + e), key0, key1).x < tau;
        pf = test ? fmaf(b, pf, a) : 0.f;
        yf = test ? yf : 0.f;
        cnt += test;
      }
      double yv = yf, r = (double)yf - pf;
      double ar = fabs(r);
      s_ape[e] += ar / fmax(fabs(yv), MAPE_EPS);
      ss_res[e] = fma(r, r, ss_res[e]);
      s_y[e] += yv;
      s_yy[e] = fma(yv, yv, s_yy[e]);
      max_res = fmax(max_res, ar);
    }
  }
  for (long long j = n4 + i; j < n; j += stride) {
    float yf = y[j], pf = x[j];
    if (SPLIT) {
      const bool test =
          philox4x32((unsigned long long)j, key0, key1).x < tau;
      pf = test ? fmaf(b, pf, a) : 0.f;
      yf = test ? yf : 0.f;
      cnt += test;
    }
    double yv = yf, r = yv - pf;
    double ar = fabs(r);
    s_ape[0] += ar / fmax(fabs(yv), MAPE_EPS);
    ss_res[0] = fma(r, r, ss_res[0]);
    s_y[0] += yv;
    s_yy[0] = fma(yv, yv, s_yy[0]);
    max_res = fmax(max_res, ar);
  }
#pragma unroll
  for (int e = 1; e < 4; ++e) {
    s_ape[0] += s_ape[e]; ss_res[0] += ss_res[e];
    s_y[0] += s_y[e]; s_yy[0] += s_yy[e];
  }
  constexpr int K = SPLIT ? 6 : 5;
  double* row = ws + (long long)blockIdx.x * K;
  __shared__ double lds[RED_WAVES];
  double t;
  if (SPLIT) {
    t = block_sum_f64<RED_WAVES>((double)cnt, lds);
    if (threadIdx.x == 0) *row++ = t;
  }
  t = block_sum_f64<RED_WAVES>(s_ape[0], lds);
  if (threadIdx.x == 0) row[0] = t;
  t = block_sum_f64<RED_WAVES>(ss_res[0], lds);
  if (threadIdx.x == 0) row[1] = t;
  t = block_sum_f64<RED_WAVES>(s_y[0], lds);
  if (threadIdx.x == 0) row[2] = t;
  t = block_sum_f64<RED_WAVES>(s_yy[0], lds);
  if (threadIdx.x == 0) row[3] = t;
  t = block_max_f64<RED_WAVES>(max_res, lds);
  if (threadIdx.x == 0) row[4] = t;
}

at::Tensor regression_metrics_hip(const at::Tensor& y,
                                  const at::Tensor& yhat) {
  TORCH_CHECK(y.is_cuda() && yhat.is_cuda() && y.numel() == yhat.numel());
  long long n = y.numel();
  auto yf = y.scalar_type() == at::kFloat ? y : y.to(at::kFloat);
  auto pf = yhat.scalar_type() == at::kFloat ? yhat : yhat.to(at::kFloat);
  const int grid = reduce_grid(n);
  auto ws = at::empty({(long long)grid * 5}, y.options().dtype(at::kDouble));
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL((regression_metrics_kernel<false>), dim3(grid),
                     dim3(RED_BLOCK), 0, stream, yf.data_ptr<float>(),
                     pf.data_ptr<float>(), (const float*)nullptr,
                     ws.data_ptr<double>(), n, 0u, 0u, 0u);
  return reduce_finalize(ws, grid, 5, 1u << 4, 1, (double)n, stream);
}

// [n_test, sum_ape, ss_res, sum_y, sum_yy, max_resid] of the linear model
// ab = [intercept, coef] over the TEST rows of random_split(x, y,
// test_frac, seed): split, predict and regression_metrics in one pass.
at::Tensor linear_split_metrics_hip(const at::Tensor& x, const at::Tensor& y,
                                    const at::Tensor& ab, double test_frac,
                                    int64_t seed) {
  TORCH_CHECK(x.is_cuda() && y.is_cuda() && x.numel() == y.numel());
  TORCH_CHECK(x.scalar_type() == at::kFloat && y.scalar_type() == at::kFloat);
  TORCH_CHECK(ab.is_cuda() && ab.numel() == 2 &&
              ab.scalar_type() == at::kFloat);
  long long n = x.numel();
  unsigned int key0, key1, tau;
  split_keys(seed, test_frac, &key0, &key1, &tau);
  const int grid = reduce_grid(n);
  auto ws = at::empty({(long long)grid * 6}, x.options().dtype(at::kDouble));
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL((regression_metrics_kernel<true>), dim3(grid),
                     dim3(RED_BLOCK), 0, stream, y.data_ptr<float>(),
                     x.data_ptr<float>(), ab.data_ptr<float>(),
                     ws.data_ptr<double>(), n, key0, key1, tau);
  return reduce_finalize(ws, grid, 6, 1u << 5, 0, 0.0, stream);
}

// ---- score_label_metrics (online: stage_4:87-113 semantics) ---------------
// out = [n, sum_ape, max_ape, s_s, s_l, s_ss, s_ll, s_sl]

__global__ void score_label_metrics_kernel(const float* __restrict__ s,
                                           const float* __restrict__ l,
                                           double* __restrict__ ws,
                                           long long n) {
  double s_ape[4] = {0, 0, 0, 0}, s_s[4] = {0, 0, 0, 0};
  double s_l[4] = {0, 0, 0, 0}, s_ss[4] = {0, 0, 0, 0};
  double s_ll[4] = {0, 0, 0, 0}, s_sl[4] = {0, 0, 0, 0};
  double max_ape = 0;
  const long long stride = (long long)gridDim.x * RED_BLOCK;
  const long long i = (long long)blockIdx.x * RED_BLOCK + threadIdx.x;
  const long long n4 = n & ~3ll;
  for (long long j = i * 4; j < n4; j += stride * 4) {
    float4 sv4 = *(const float4*)(s + j);
    float4 lv4 = *(const float4*)(l + j);
    const float ss4[4] = {sv4.x, sv4.y, sv4.z, sv4.w};
    const float ll4[4] = {lv4.x, lv4.y, lv4.z, lv4.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      double sv = ss4[e], lv = ll4[e];
      double ape = fabs(sv / lv - 1.0);  // reference has no eps guard
      s_ape[e] += ape;
      max_ape = fmax(max_ape, ape);
      s_s[e] += sv;
      s_l[e] += lv;
      s_ss[e] = fma(sv, sv, s_ss[e]);
      s_ll[e] = fma(lv, lv, s_ll[e]);
      s_sl[e] = fma(sv, lv, s_sl[e]);
    }
  }
  for (long long j = n4 + i; j < n; j += stride) {
    double sv = s[j], lv = l[j];
    double ape = fabs(sv / lv - 1.0);
    s_ape[0] += ape;
    max_ape = fmax(max_ape, ape);
    s_s[0] += sv; s_l[0] += lv;
    s_ss[0] = fma(sv, sv, s_ss[0]);
    s_ll[0] = fma(lv, lv, s_ll[0]);
    s_sl[0] = fma(sv, lv, s_sl[0]);
  }
#pragma unroll
  for (int e = 1; e < 4; ++e) {
    s_ape[0] += s_ape[e]; s_s[0] += s_s[e]; s_l[0] += s_l[e];
    s_ss[0] += s_ss[e]; s_ll[0] += s_ll[e]; s_sl[0] += s_sl[e];
  }
  double* row = ws + (long long)blockIdx.x * 7;
  __shared__ double lds[RED_WAVES];
  double t;
  // ws row = [sum_ape, max_ape, s_s, s_l, s_ss, s_ll, s_sl] (out[1..7])
  t = block_sum_f64<RED_WAVES>(s_ape[0], lds);
  if (threadIdx.x == 0) row[0] = t;
  t = block_max_f64<RED_WAVES>(max_ape, lds);
  if (threadIdx.x == 0) row[1] = t;
  t = block_sum_f64<RED_WAVES>(s_s[0], lds);
  if (threadIdx.x == 0) row[2] = t;
  t = block_sum_f64<RED_WAVES>(s_l[0], lds);
  if (threadIdx.x == 0) row[3] = t;
  t = block_sum_f64<RED_WAVES>(s_ss[0], lds);
  if (threadIdx.x == 0) row[4] = t;
  t = block_sum_f64<RED_WAVES>(s_ll[0], lds);
  if (threadIdx.x == 0) row[5] = t;
  t = block_sum_f64<RED_WAVES>(s_sl[0], lds);
  if (threadIdx.x == 0) row[6] = t;
}

at::Tensor score_label_metrics_hip(const at::Tensor& s, const at::Tensor& l) {
  TORCH_CHECK(s.is_cuda() && l.is_cuda() && s.numel() == l.numel());
  long long n = s.numel();
  auto sf = s.scalar_type() == at::kFloat ? s : s.to(at::kFloat);
  auto lf = l.scalar_type() == at::kFloat ? l : l.to(at::kFloat);
  const int grid = reduce_grid(n);
  auto ws = at::empty({(long long)grid * 7}, s.options().dtype(at::kDouble));
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(score_label_metrics_kernel, dim3(grid),
                     dim3(RED_BLOCK), 0, stream, sf.data_ptr<float>(),
                     lf.data_ptr<float>(), ws.data_ptr<double>(), n);
  return reduce_finalize(ws, grid, 7, 1u << 1, 1, (double)n, stream);
}
