// resid_select: exact order statistics of |label - score| on the device —
// gfx950.  The conformal half-width of a hold-out is the k-th smallest
// absolute residual; this finds it with RS_PASSES streaming histogram passes
// and no sort.  The key rule, the rank, the passes and the state are in
// resid_select.h.
//
// The pass and the pick are separate ops so that the caller may all-reduce
// the histogram between them (histograms of row shards add):
//   resid_select_pass(a, b, state, pass, nq, ab?, test_frac, seed) -> int64
//       [1, RS_W0] (pass 0) or [nq, RS_BINS]
//   resid_select_pick(hist, state, pass, levels) -> fp32 [nq]
// Rows: plain (ab absent) (a, b) = (labels, scores), every row; split-linear
// (ab given) (a, b) = (y, x), the TEST rows of random_split(x, y, test_frac,
// seed) scored by the linear model ab = [intercept, coef].
#include <ATen/cuda/CUDAContext.h>
#include <hip/hip_runtime.h>
#include <torch/extension.h>

#include <algorithm>
#include <cstdint>

#include "resid_select.h"

// 4 blocks per CU, the cap drift_histograms measured for the same loop
#define RS_GRID_CAP 1024

static void check_state(const at::Tensor& state, const char* op) {
  TORCH_CHECK(state.is_cuda() && state.scalar_type() == at::kLong &&
                  state.is_contiguous() && state.numel() == RS_STATE,
              op, ": state is a contiguous int64[", RS_STATE,
              "] device tensor");
}

template <bool PASS0, bool SPLIT>
static void launch_pass(const float* ap, const float* bp,
                        const long long* state, unsigned int* ws, long long n,
                        int pass, int nq, int grid, size_t lds,
                        const ResidRows<SPLIT>& src, hipStream_t stream) {
  // a view such as t[1:] is contiguous but not 16-byte aligned
  const bool vec = (((uintptr_t)ap | (uintptr_t)bp) & 15) == 0;
  if (vec)
    hipLaunchKernelGGL((resid_select_pass_kernel<PASS0, SPLIT, true>),
                       dim3(grid), dim3(DH_BLOCK), lds, stream, ap, bp, state,
                       ws, n, pass, nq, src);
  else
    hipLaunchKernelGGL((resid_select_pass_kernel<PASS0, SPLIT, false>),
                       dim3(grid), dim3(DH_BLOCK), lds, stream, ap, bp, state,
                       ws, n, pass, nq, src);
}

at::Tensor resid_select_pass_hip(const at::Tensor& a, const at::Tensor& b,
                                 const at::Tensor& state, int64_t pass,
                                 int64_t nq,
                                 const c10::optional<at::Tensor>& ab,
                                 double test_frac, int64_t seed) {
  TORCH_CHECK(a.is_cuda() && b.is_cuda(),
              "resid_select_pass: tensors must be on the GPU");
  TORCH_CHECK(a.scalar_type() == at::kFloat && b.scalar_type() == at::kFloat,
              "resid_select_pass: tensors must be float32");
  TORCH_CHECK(a.is_contiguous() && b.is_contiguous(),
              "resid_select_pass: tensors must be contiguous");
  TORCH_CHECK(a.numel() == b.numel(),
              "resid_select_pass: the two inputs differ in length");
  TORCH_CHECK(pass >= 0 && pass < RS_PASSES, "resid_select_pass: 0 <= pass < ",
              RS_PASSES);
  TORCH_CHECK(nq >= 1 && nq <= RS_MAXQ, "resid_select_pass: 1 <= levels <= ",
              RS_MAXQ);
  check_state(state, "resid_select_pass");
  const bool split = ab.has_value();
  if (split)
    TORCH_CHECK(ab->is_cuda() && ab->numel() == 2 &&
                    ab->scalar_type() == at::kFloat && ab->is_contiguous(),
                "resid_select_pass: ab is a float32[2] device tensor");

  const long long n = a.numel();
  const int tabs = pass == 0 ? 1 : (int)nq;
  const int Wt = pass == 0 ? RS_W0 : RS_BINS;
  const int W = tabs * Wt;
  auto opts = a.options().dtype(at::kLong);
  if (n == 0) return at::zeros({tabs, Wt}, opts);

  const long long per_sweep = (long long)DH_BLOCK * 4;
  const int grid = (int)std::max<long long>(
      std::min<long long>((n + per_sweep - 1) / per_sweep, RS_GRID_CAP), 1);
  // a block's partial counts are uint32: rows per block = sweeps * 1024
  const long long sweeps = (n + per_sweep * grid - 1) / (per_sweep * grid);
  TORCH_CHECK(sweeps * per_sweep < (1ll << 32), "resid_select_pass: ", n,
              " rows overflow a block's uint32 counts");

  auto ws = at::empty({(long long)grid * W}, a.options().dtype(at::kInt));
  auto out = at::empty({tabs, Wt}, opts);
  auto stream = at::cuda::getCurrentCUDAStream();
  const float* ap = a.data_ptr<float>();
  const float* bp = b.data_ptr<float>();
  const long long* sp = (const long long*)state.data_ptr<int64_t>();
  unsigned int* wsp = (unsigned int*)ws.data_ptr<int32_t>();
  const size_t lds = (size_t)DH_WAVES * W * sizeof(unsigned int);
  if (split) {
    const ResidRows<true> src{ab->data_ptr<float>(),
                              split_key(seed, test_frac)};
    if (pass == 0)
      launch_pass<true, true>(ap, bp, sp, wsp, n, 0, (int)nq, grid, lds, src,
                              stream);
    else
      launch_pass<false, true>(ap, bp, sp, wsp, n, (int)pass, (int)nq, grid,
                               lds, src, stream);
  } else {
    const ResidRows<false> src{};
    if (pass == 0)
      launch_pass<true, false>(ap, bp, sp, wsp, n, 0, (int)nq, grid, lds, src,
                               stream);
    else
      launch_pass<false, false>(ap, bp, sp, wsp, n, (int)pass, (int)nq, grid,
                                lds, src, stream);
  }
  hipLaunchKernelGGL(drift_hist_finalize,
                     dim3((W + DH_FIN_SLOTS - 1) / DH_FIN_SLOTS),
                     dim3(DH_BLOCK), 0, stream, wsp,
                     (long long*)out.data_ptr<int64_t>(), grid, W);
  return out;
}

at::Tensor resid_select_pick_hip(const at::Tensor& hist, at::Tensor state,
                                 int64_t pass, at::ArrayRef<double> levels) {
  TORCH_CHECK(pass >= 0 && pass < RS_PASSES, "resid_select_pick: 0 <= pass < ",
              RS_PASSES);
  const int nq = (int)levels.size();
  TORCH_CHECK(nq >= 1 && nq <= RS_MAXQ, "resid_select_pick: 1 <= levels <= ",
              RS_MAXQ);
  check_state(state, "resid_select_pick");
  TORCH_CHECK(hist.is_cuda() && hist.scalar_type() == at::kLong &&
                  hist.is_contiguous() &&
                  hist.numel() == (pass == 0 ? RS_W0 : nq * RS_BINS),
              "resid_select_pick: hist is the contiguous int64 table of "
              "resid_select_pass for this pass and these levels");
  ResidLevels lv{};
  for (int q = 0; q < nq; ++q) {
    TORCH_CHECK(levels[q] > 0.0 && levels[q] < 1.0,
                "resid_select_pick: a level lies in (0, 1)");
    lv.L[q] = levels[q];
  }
  auto out = at::empty({nq}, hist.options().dtype(at::kFloat));
  hipLaunchKernelGGL(resid_select_pick_kernel, dim3(1), dim3(DH_BLOCK), 0,
                     at::cuda::getCurrentCUDAStream(),
                     (const long long*)hist.data_ptr<int64_t>(),
                     (long long*)state.data_ptr<int64_t>(),
                     out.data_ptr<float>(), (int)pass, nq, lv);
  return out;
}
