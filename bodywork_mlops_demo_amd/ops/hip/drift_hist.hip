// drift_histograms: fused device histograms for the data-drift monitor —
// gfx950.
//
// One 12 B/row pass over (x, labels, scores) bins the three arrays and the
// residual labels - scores, the four distributions PSI / KS are computed
// from (monitoring/drift.py).  Returns int64 [4, bins + 3]: rows x, labels,
// scores, residual; slot 0 underflow, 1..bins the bins, bins + 1 overflow,
// bins + 2 NaN.  The slot rule and the two kernels are in drift_hist.h.
#include <ATen/cuda/CUDAContext.h>
#include <hip/hip_runtime.h>
#include <torch/extension.h>

#include <algorithm>
#include <cstdint>

#include "drift_hist.h"

// Stage-1 grid cap, chosen by measurement (profiles/drift_histograms.md):
// 4 blocks per CU; 512 and 2048 are slower at 10M and at 100M rows.
#define DH_GRID_CAP 1024

at::Tensor drift_histograms_hip(const at::Tensor& x, const at::Tensor& labels,
                                const at::Tensor& scores, int64_t bins,
                                at::ArrayRef<double> lo,
                                at::ArrayRef<double> scale) {
  TORCH_CHECK(x.is_cuda() && labels.is_cuda() && scores.is_cuda(),
              "drift_histograms: tensors must be on the GPU");
  TORCH_CHECK(x.scalar_type() == at::kFloat &&
                  labels.scalar_type() == at::kFloat &&
                  scores.scalar_type() == at::kFloat,
              "drift_histograms: tensors must be float32");
  TORCH_CHECK(x.is_contiguous() && labels.is_contiguous() &&
                  scores.is_contiguous(),
              "drift_histograms: tensors must be contiguous");
  TORCH_CHECK(x.numel() == labels.numel() && x.numel() == scores.numel(),
              "drift_histograms: x, labels and scores differ in length");
  TORCH_CHECK(bins >= 1 && bins <= DH_MAX_BINS, "drift_histograms: 1 <= bins <= ",
              DH_MAX_BINS);
  TORCH_CHECK(lo.size() == DH_ROWS && scale.size() == DH_ROWS,
              "drift_histograms: lo and scale take one value per row (4)");
  DriftBins p;
  for (int k = 0; k < DH_ROWS; ++k) {
    // fp32 values handed down as doubles: the casts are exact
    p.lo[k] = (float)lo[k];
    p.scale[k] = (float)scale[k];
  }
  const long long n = x.numel();
  const int S = (int)bins + 3;
  const int W = DH_ROWS * S;
  auto opts = x.options().dtype(at::kLong);
  if (n == 0) return at::zeros({DH_ROWS, S}, opts);

  const long long per_sweep = (long long)DH_BLOCK * 4;
  const int grid = (int)std::max<long long>(
      std::min<long long>((n + per_sweep - 1) / per_sweep, DH_GRID_CAP), 1);
  // a block's partial counts are uint32: rows per block = sweeps * 1024
  const long long sweeps = (n + per_sweep * grid - 1) / (per_sweep * grid);
  TORCH_CHECK(sweeps * per_sweep < (1ll << 32),
              "drift_histograms: ", n, " rows overflow a block's uint32 counts");

  auto ws = at::empty({(long long)grid * W}, x.options().dtype(at::kInt));
  auto out = at::empty({DH_ROWS, S}, opts);
  auto stream = at::cuda::getCurrentCUDAStream();
  const float* xp = x.data_ptr<float>();
  const float* lp = labels.data_ptr<float>();
  const float* sp = scores.data_ptr<float>();
  unsigned int* wsp = (unsigned int*)ws.data_ptr<int32_t>();
  // a view such as t[1:] is contiguous but not 16-byte aligned
  const bool vec = (((uintptr_t)xp | (uintptr_t)lp | (uintptr_t)sp) & 15) == 0;
  if (vec)
    hipLaunchKernelGGL((drift_hist_kernel<true>), dim3(grid), dim3(DH_BLOCK),
                       0, stream, xp, lp, sp, wsp, n, (int)bins, p);
  else
    hipLaunchKernelGGL((drift_hist_kernel<false>), dim3(grid), dim3(DH_BLOCK),
                       0, stream, xp, lp, sp, wsp, n, (int)bins, p);
  hipLaunchKernelGGL(drift_hist_finalize,
                     dim3((W + DH_FIN_SLOTS - 1) / DH_FIN_SLOTS),
                     dim3(DH_BLOCK), 0, stream, wsp,
                     (long long*)out.data_ptr<int64_t>(), grid, W);
  return out;
}
