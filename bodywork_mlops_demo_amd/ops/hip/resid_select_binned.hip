// resid_select_binned: per-cell exact order statistics of |label - score|
// and the coverage of the x-dependent band they make — gfx950.  Cell rule,
// passes, LDS layout and state are in resid_select_binned.h.
//
// Pass and pick are separate ops so that the caller may all-reduce the
// histogram between them (histograms of row shards add):
//   resid_select_binned_pass(x, a, b?, state, pass, nq, cells, lo, scale,
//       ab?, test_frac, seed) -> int64 [cells * 256 + 4] (pass 0) or
//       [cells, nq, 256]
//   resid_select_binned_pick(hist, state, pass, levels, cells)
//       -> fp32 [cells, nq]
//   binned_interval_coverage(x, s, l, halfwidths[cells, 4], cells, lo, scale)
//       -> int64 [cells, 5]
// Rows: plain (ab absent) x, a = labels, b = scores, every row; split-linear
// (ab given, b absent) a = y, the TEST rows of random_split(x, y, test_frac,
// seed) scored by the linear model ab = [intercept, coef].
#include <ATen/cuda/CUDAContext.h>
#include <hip/hip_runtime.h>
#include <torch/extension.h>

#include <algorithm>
#include <cstdint>

#include "resid_select_binned.h"

static BinCells check_cells(int64_t cells, double lo, double scale,
                            const char* op) {
  TORCH_CHECK(cells >= 1 && cells <= BS_MAXC, op, ": 1 <= cells <= ", BS_MAXC);
  TORCH_CHECK((float)scale > 0.f, op, ": the cell scale is positive");
  return BinCells{(int)cells, (float)lo, (float)scale};
}

static void check_binned_state(const at::Tensor& state, int cells, int nq,
                               const char* op) {
  TORCH_CHECK(state.is_cuda() && state.scalar_type() == at::kLong &&
                  state.is_contiguous() &&
                  state.numel() == (int64_t)cells * bs_state_row(nq),
              op, ": state is a contiguous int64 [cells, 2 + 3 * levels] "
                  "device tensor");
}

static bool aligned16(const float* p) { return ((uintptr_t)p & 15) == 0; }

// blocks for n rows, and the check that a block's uint32 counts hold them
static int binned_grid(long long n, const char* op) {
  const long long per_sweep = (long long)BS_BLOCK * 4;
  const int grid = (int)std::max<long long>(
      std::min<long long>((n + per_sweep - 1) / per_sweep, BS_GRID_CAP), 1);
  const long long sweeps = (n + per_sweep * grid - 1) / (per_sweep * grid);
  TORCH_CHECK(sweeps * per_sweep < (1ll << 32), op, ": ", n,
              " rows overflow a block's uint32 counts");
  return grid;
}

template <bool PASS0, bool SPLIT, bool VEC>
static void launch_binned(const float* x, const float* a, const float* b,
                          const long long* state, unsigned int* ws,
                          long long n, int pass, int nq, int grid, size_t lds,
                          int copies, const BinCells& g, const ResidRows<SPLIT>& src,
                          hipStream_t stream) {
  auto kernel = resid_select_binned_pass_kernel<PASS0, SPLIT, VEC>;
  // more than 64 KB of LDS (the tables and the static prefixes) is opt-in
  if (lds + sizeof(uint4) * BS_MAXC > 64 * 1024) {
    static const hipError_t attr = hipFuncSetAttribute(
        (const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
        160 * 1024 - (int)sizeof(uint4) * BS_MAXC);
    TORCH_CHECK(attr == hipSuccess, "resid_select_binned_pass: ",
                hipGetErrorString(attr));
  }
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(BS_BLOCK), lds, stream, x, a, b,
                     state, ws, n, pass, nq, copies, g, src);
}

template <bool SPLIT>
static void launch_binned_pass(const float* x, const float* a, const float* b,
                               const long long* state, unsigned int* ws,
                               long long n, int pass, int nq, int grid,
                               size_t lds, int copies, const BinCells& g,
                               const ResidRows<SPLIT>& src,
                               hipStream_t stream) {
  // a view such as t[1:] is contiguous but not 16-byte aligned
  const bool vec = aligned16(x) && aligned16(a) && (SPLIT || aligned16(b));
#define BS_LAUNCH(P0, V)                                                    \
  launch_binned<P0, SPLIT, V>(x, a, b, state, ws, n, pass, nq, grid, lds, \
                              copies, g, src, stream)
  if (pass == 0) {
    if (vec) BS_LAUNCH(true, true); else BS_LAUNCH(true, false);
  } else {
    if (vec) BS_LAUNCH(false, true); else BS_LAUNCH(false, false);
  }
#undef BS_LAUNCH
}

at::Tensor resid_select_binned_pass_hip(
    const at::Tensor& x, const at::Tensor& a,
    const c10::optional<at::Tensor>& b, const at::Tensor& state, int64_t pass,
    int64_t nq, int64_t cells, double lo, double scale,
    const c10::optional<at::Tensor>& ab, double test_frac, int64_t seed) {
  const char* op = "resid_select_binned_pass";
  const bool split = ab.has_value();
  TORCH_CHECK(split != b.has_value(), op,
              ": give scores (plain) or ab (split-linear), not both");
  const at::Tensor& b_ = split ? x : *b;
  TORCH_CHECK(x.is_cuda() && a.is_cuda() && b_.is_cuda(), op,
              ": tensors must be on the GPU");
  TORCH_CHECK(x.scalar_type() == at::kFloat && a.scalar_type() == at::kFloat &&
                  b_.scalar_type() == at::kFloat,
              op, ": tensors must be float32");
  TORCH_CHECK(x.is_contiguous() && a.is_contiguous() && b_.is_contiguous(), op,
              ": tensors must be contiguous");
  TORCH_CHECK(x.numel() == a.numel() && x.numel() == b_.numel(), op,
              ": the inputs differ in length");
  TORCH_CHECK(pass >= 0 && pass < BS_PASSES, op, ": 0 <= pass < ", BS_PASSES);
  TORCH_CHECK(nq >= 1 && nq <= BS_MAXQ, op, ": 1 <= levels <= ", BS_MAXQ);
  const BinCells g = check_cells(cells, lo, scale, op);
  check_binned_state(state, g.n, (int)nq, op);
  if (split)
    TORCH_CHECK(ab->is_cuda() && ab->numel() == 2 &&
                    ab->scalar_type() == at::kFloat && ab->is_contiguous(),
                op, ": ab is a float32[2] device tensor");

  const long long n = x.numel();
  const int W = pass == 0 ? g.n * BS_BINS + 4 : g.n * (int)nq * BS_BINS;
  auto opts = x.options().dtype(at::kLong);
  auto shape = pass == 0 ? std::vector<int64_t>{W}
                         : std::vector<int64_t>{g.n, nq, BS_BINS};
  if (n == 0) return at::zeros(shape, opts);

  const int grid = binned_grid(n, op);
  auto ws = at::empty({(long long)grid * W}, x.options().dtype(at::kInt));
  auto out = at::empty(shape, opts);
  auto stream = at::cuda::getCurrentCUDAStream();
  const long long* sp = (const long long*)state.data_ptr<int64_t>();
  unsigned int* wsp = (unsigned int*)ws.data_ptr<int32_t>();
  const int copies = pass == 0 ? BS_COPIES : 1;
  const size_t lds = (size_t)copies * W * sizeof(unsigned int);
  if (split) {
    const ResidRows<true> src{ab->data_ptr<float>(),
                              split_key(seed, test_frac)};
    launch_binned_pass<true>(x.data_ptr<float>(), a.data_ptr<float>(), nullptr,
                             sp, wsp, n, (int)pass, (int)nq, grid, lds, copies, g,
                             src, stream);
  } else {
    const ResidRows<false> src{};
    launch_binned_pass<false>(x.data_ptr<float>(), a.data_ptr<float>(),
                              b_.data_ptr<float>(), sp, wsp, n, (int)pass,
                              (int)nq, grid, lds, copies, g, src, stream);
  }
  hipLaunchKernelGGL(drift_hist_finalize,
                     dim3((W + DH_FIN_SLOTS - 1) / DH_FIN_SLOTS),
                     dim3(DH_BLOCK), 0, stream, wsp,
                     (long long*)out.data_ptr<int64_t>(), grid, W);
  return out;
}

at::Tensor resid_select_binned_pick_hip(const at::Tensor& hist,
                                        at::Tensor state, int64_t pass,
                                        at::ArrayRef<double> levels,
                                        int64_t cells) {
  const char* op = "resid_select_binned_pick";
  TORCH_CHECK(pass >= 0 && pass < BS_PASSES, op, ": 0 <= pass < ", BS_PASSES);
  const int nq = (int)levels.size();
  TORCH_CHECK(nq >= 1 && nq <= BS_MAXQ, op, ": 1 <= levels <= ", BS_MAXQ);
  TORCH_CHECK(cells >= 1 && cells <= BS_MAXC, op, ": 1 <= cells <= ", BS_MAXC);
  check_binned_state(state, (int)cells, nq, op);
  TORCH_CHECK(hist.is_cuda() && hist.scalar_type() == at::kLong &&
                  hist.is_contiguous() &&
                  hist.numel() == (pass == 0 ? cells * BS_BINS + 4
                                             : cells * nq * BS_BINS),
              op, ": hist is the contiguous int64 table of "
                  "resid_select_binned_pass for this pass, these levels and "
                  "these cells");
  ResidLevels lv{};
  for (int q = 0; q < nq; ++q) {
    TORCH_CHECK(levels[q] > 0.0 && levels[q] < 1.0, op,
                ": a level lies in (0, 1)");
    lv.L[q] = levels[q];
  }
  auto out = at::empty({cells, nq}, hist.options().dtype(at::kFloat));
  hipLaunchKernelGGL(resid_select_binned_pick_kernel, dim3((int)cells),
                     dim3(BS_BINS), 0, at::cuda::getCurrentCUDAStream(),
                     (const long long*)hist.data_ptr<int64_t>(),
                     (long long*)state.data_ptr<int64_t>(),
                     out.data_ptr<float>(), (int)pass, nq, lv);
  return out;
}

at::Tensor binned_interval_coverage_hip(const at::Tensor& x,
                                        const at::Tensor& s,
                                        const at::Tensor& l,
                                        const at::Tensor& halfwidths,
                                        int64_t cells, double lo,
                                        double scale) {
  const char* op = "binned_interval_coverage";
  TORCH_CHECK(x.is_cuda() && s.is_cuda() && l.is_cuda(), op,
              ": tensors must be on the GPU");
  TORCH_CHECK(x.scalar_type() == at::kFloat && s.scalar_type() == at::kFloat &&
                  l.scalar_type() == at::kFloat && x.is_contiguous() &&
                  s.is_contiguous() && l.is_contiguous(),
              op, ": tensors must be contiguous float32");
  TORCH_CHECK(x.numel() == s.numel() && x.numel() == l.numel(), op,
              ": the inputs differ in length");
  const BinCells g = check_cells(cells, lo, scale, op);
  TORCH_CHECK(halfwidths.is_cuda() && halfwidths.scalar_type() == at::kFloat &&
                  halfwidths.is_contiguous() &&
                  halfwidths.numel() == cells * BS_MAXQ,
              op, ": halfwidths is a float32 [cells, 4] device tensor "
                  "(unused levels -1)");
  const long long n = x.numel();
  auto opts = x.options().dtype(at::kLong);
  if (n == 0) return at::zeros({cells, 1 + BS_MAXQ}, opts);

  const int W = g.n * BS_MASKS;
  const int grid = binned_grid(n, op);
  auto ws = at::empty({(long long)grid * W}, x.options().dtype(at::kInt));
  auto masks = at::empty({W}, opts);
  auto out = at::empty({cells, 1 + BS_MAXQ}, opts);
  auto stream = at::cuda::getCurrentCUDAStream();
  const float* xp = x.data_ptr<float>();
  const float* sp = s.data_ptr<float>();
  const float* lp = l.data_ptr<float>();
  unsigned int* wsp = (unsigned int*)ws.data_ptr<int32_t>();
  if (aligned16(xp) && aligned16(sp) && aligned16(lp))
    hipLaunchKernelGGL(binned_coverage_kernel<true>, dim3(grid),
                       dim3(BS_BLOCK), 0, stream, xp, sp, lp,
                       halfwidths.data_ptr<float>(), wsp, n, g);
  else
    hipLaunchKernelGGL(binned_coverage_kernel<false>, dim3(grid),
                       dim3(BS_BLOCK), 0, stream, xp, sp, lp,
                       halfwidths.data_ptr<float>(), wsp, n, g);
  hipLaunchKernelGGL(drift_hist_finalize,
                     dim3((W + DH_FIN_SLOTS - 1) / DH_FIN_SLOTS),
                     dim3(DH_BLOCK), 0, stream, wsp,
                     (long long*)masks.data_ptr<int64_t>(), grid, W);
  hipLaunchKernelGGL(binned_coverage_fold_kernel, dim3(1),
                     dim3(BS_MAXC * (1 + BS_MAXQ)), 0, stream,
                     (const long long*)masks.data_ptr<int64_t>(),
                     (long long*)out.data_ptr<int64_t>(), g.n);
  return out;
}
