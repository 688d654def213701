"""Two-stage deterministic reductions and the fused split-aware linear fit.

Every reduction op writes per-block partials and combines them in a
second, fixed-order kernel, so besides matching the CPU oracles the
results must be bitwise equal from call to call.  The fused ops
(``linreg_split_stats`` / ``linear_split_metric_sums``) must see exactly
the rows ``random_split`` would hand to the unfused path.

Sizes: 1 / 3 (scalar tail only), 255 / 256 / 257 (one block, float4 body
+ tail), 1027 (two blocks), 2^20+3 (the full 1024-block grid, one sweep
of 4 rows per thread, plus a tail) and 3*2^20+5 (three grid-stride
sweeps).  Rows come from ``ops.datagen(n, 1, seed)`` — one generation,
sliced from row 0 so every size keeps the buffer's 16-byte alignment.

Tolerances are the ones tests/test_ops_gpu.py uses for the same ops:
rtol=1e-12 (atol=1e-6) for statistics, rel=1e-9 for metrics.  The atol
covers the polynomial statistics whose odd-power terms cancel: fp64 tree
summation of <= 3.2e6 terms with |term| <= 100 is off by at most
eps * log2(n) * sum|term| = 1.1e-16 * 22 * 3.2e8 = 7.7e-7.
"""
import functools

import pytest
import torch

from bodywork_mlops_demo_amd import ops
from bodywork_mlops_demo_amd.models import GPULinearRegressor
from bodywork_mlops_demo_amd.ops import reference

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES = [1, 3, 255, 256, 257, 1027, (1 << 20) + 3, 3 * (1 << 20) + 5]
# not exactly representable products: the CPU oracle's mul+add and the
# kernels' fmaf may differ by one fp32 ulp per prediction
A, B = 1.1, 0.47


@pytest.fixture(scope="module")
def data():
    assert ops.hip_available()
    n_max = max(SIZES)
    y, X = ops.datagen(n_max + n_max // 8, 1, seed=20260101, device=DEV)
    assert y.shape[0] >= n_max  # the y>=0 cull removes a few percent
    X, y = X[:n_max].contiguous(), y[:n_max].contiguous()
    torch.cuda.synchronize()
    return X, y, X.cpu(), y.cpu()


@pytest.fixture(scope="module")
def oracle(data):
    """CPU oracles, computed once per (kind, n, ...) and shared."""
    _, _, Xc, yc = data

    @functools.lru_cache(maxsize=None)
    def split(n, frac, seed):
        return reference.random_split_cpu(Xc[:n], yc[:n], frac, seed)

    @functools.lru_cache(maxsize=None)
    def get(kind, n, *args):
        X, y = Xc[:n], yc[:n]
        if kind == "linreg":
            return reference.linreg_stats_cpu(X, y)
        if kind == "poly":
            return reference.poly_stats_cpu(X, y, 4, 50.0, 50.0)
        if kind == "split_stats":
            X_tr, y_tr, _, _ = split(n, *args)
            return reference.linreg_stats_cpu(X_tr, y_tr)
        if kind == "split_metrics":
            _, _, X_te, y_te = split(n, *args)
            if X_te.numel() == 0:  # empty test partition: all sums zero
                return (0.0,) * 6
            yhat = reference.linear_score_cpu(X_te, A, B)
            return reference.metric_sums_cpu(y_te, yhat)
        raise KeyError(kind)

    return get


def _approx_each(got, want, rel):
    got, want = list(map(float, got)), list(map(float, want))
    print("got ", got)
    print("want", want)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == pytest.approx(w, rel=rel)


@pytest.mark.parametrize("n", SIZES)
def test_linreg_stats(data, oracle, n):
    X, y = data[0][:n], data[1][:n]
    got = ops.linreg_stats(X, y)
    torch.testing.assert_close(got.cpu(), oracle("linreg", n),
                               rtol=1e-12, atol=1e-6)
    assert torch.equal(got, ops.linreg_stats(X, y))


@pytest.mark.parametrize("n", SIZES)
def test_poly_stats(data, oracle, n):
    X, y = data[0][:n], data[1][:n]
    got = ops.poly_stats(X, y, degree=3)
    torch.testing.assert_close(got.cpu(), oracle("poly", n),
                               rtol=1e-12, atol=1e-6)
    assert torch.equal(got, ops.poly_stats(X, y, degree=3))


@pytest.mark.parametrize("n", SIZES)
def test_regression_metrics(data, n):
    X, y = data[0][:n], data[1][:n]
    yhat = ops.linear_score(X, A, B)
    got = ops.regression_metric_sums(y, yhat)
    want = reference.metric_sums_cpu(y.cpu(), yhat.cpu())
    _approx_each(got.cpu(), want, rel=1e-9)
    assert torch.equal(got, ops.regression_metric_sums(y, yhat))
    m = ops.regression_metrics(y, yhat)
    assert m["MAPE"] == pytest.approx(want[1] / want[0], rel=1e-9)
    assert m["max_residual"] == pytest.approx(want[5], rel=1e-9)


@pytest.mark.parametrize("n", SIZES)
def test_score_label_metrics(data, n):
    X, labels = data[0][:n], data[1][:n]
    scores = ops.linear_score(X, A, B)
    got = ops.score_label_metrics(scores, labels)
    want = ops.score_label_metrics(scores.cpu(), labels.cpu())
    print("got ", got)
    print("want", want)
    for k in ("MAPE", "r_squared", "max_residual"):
        assert got[k] == pytest.approx(want[k], rel=1e-9)
    core = torch.ops.bodywork_hip
    assert torch.equal(core.score_label_metrics(scores, labels),
                       core.score_label_metrics(scores, labels))


SPLIT_CASES = [(n, 0.2, 42) for n in SIZES] + [
    (1, 0.0, 42),            # tau = 0: nobody is a test row
    (257, 0.35, 7),          # non-default seed and fraction
    ((1 << 20) + 3, 0.2, 7),
]


@pytest.mark.parametrize("n,frac,seed", SPLIT_CASES)
def test_split_stats_match_cpu_split(data, oracle, n, frac, seed):
    X, y = data[0][:n], data[1][:n]
    got = ops.linreg_split_stats(X, y, frac, seed)
    want = oracle("split_stats", n, frac, seed)
    assert float(got[0]) == float(want[0])  # n_train is exact
    torch.testing.assert_close(got.cpu(), want, rtol=1e-12, atol=1e-6)
    assert torch.equal(got, ops.linreg_split_stats(X, y, frac, seed))


@pytest.mark.parametrize("n,frac,seed", SPLIT_CASES)
def test_split_metrics_match_unfused_gpu_path(data, n, frac, seed):
    """Same rows, same fp32 predictions as random_split -> predict ->
    regression_metrics: only the fp64 summation order differs."""
    X, y = data[0][:n], data[1][:n]
    model = GPULinearRegressor(A, B, device=DEV)
    _, _, X_te, y_te = ops.random_split(X, y, frac, seed)
    want = ops.regression_metric_sums(y_te, model.predict(X_te)).cpu()
    got = ops.linear_split_metric_sums(X, y, model._ab_tensor(), frac, seed)
    assert float(got[0]) == float(X_te.shape[0])
    if n == 1:
        assert float(got[0]) == 0.0  # row 0 is a train row: empty test set
        assert got.cpu().tolist() == [0.0] * 6
    _approx_each(got.cpu(), want, rel=1e-12)
    assert float(got[5]) == float(want[5])  # a max has no rounding
    assert torch.equal(
        got, ops.linear_split_metric_sums(X, y, model._ab_tensor(), frac,
                                          seed))


@pytest.mark.parametrize("n,frac,seed", SPLIT_CASES)
def test_split_metrics_match_cpu_oracle(data, oracle, n, frac, seed):
    """yhat may differ from the oracle's by one fp32 ulp (~6e-8
    relative), so the sums agree to well inside 1e-6."""
    X, y = data[0][:n], data[1][:n]
    ab = torch.tensor([A, B], device=DEV, dtype=torch.float32)
    got = ops.linear_split_metric_sums(X, y, ab, frac, seed).cpu()
    want = oracle("split_metrics", n, frac, seed)
    assert float(got[0]) == float(want[0])
    _approx_each(got, want, rel=1e-6)


def test_fit_split_equals_unfused_fit(data):
    """GPULinearRegressor.fit_split == random_split + fit + predict +
    regression_metrics up to fp64 summation order."""
    n = (1 << 20) + 3
    X, y = data[0][:n], data[1][:n]
    fused = GPULinearRegressor(device=DEV)
    m_fused = fused.fit_split(X, y, 0.2, seed=42)
    X_tr, y_tr, X_te, y_te = ops.random_split(X, y, 0.2, seed=42)
    plain = GPULinearRegressor(device=DEV).fit(X_tr, y_tr)
    m_plain = ops.regression_metrics(y_te, plain.predict(X_te))
    # the 2x2 solve amplifies the ~1e-15 summation-order difference of the
    # statistics by at most ~1e3 (intercept ~1 against mean(y) ~26)
    assert fused.intercept_ == pytest.approx(plain.intercept_, rel=1e-10)
    assert fused.coef_ == pytest.approx(plain.coef_, rel=1e-10)
    for k in ("MAPE", "r_squared", "max_residual"):
        assert m_fused[k] == pytest.approx(m_plain[k], rel=1e-6)
