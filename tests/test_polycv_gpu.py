"""One-pass K-fold model selection on the device: the poly_fold_stats
kernel against an int64 oracle at every grid/sweep boundary, the wide
finalise against the one-block one, device selection against the CPU
path, and two polycv cycles end to end."""
import functools
from datetime import date

import numpy as np
import pytest
import torch

from bodywork_mlops_demo_amd import ops
from bodywork_mlops_demo_amd.models import GPUPolyRegressorCV
from bodywork_mlops_demo_amd.ops import reference
from polycv_data import as_f32, int64_fold_stats, integer_rows, quadratic_rows

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SWEEP = 1024 * 256  # rows one sweep of the full 1024-block grid covers
# empty folds, a partial wave, a block boundary, more than one block, the
# full grid, a second and a third grid-stride sweep
SIZES = [1, 3, 5, 255, 256, 257, 1027, SWEEP + 3, 2 * SWEEP + 5]
N_MAX = max(SIZES)

# Worst relative deviation of the device path's CV scores from the CPU
# path's on the designed quadratic rows, measured on an MI355X
# (profiles/poly_cv.md); the test allows 100x that.
SCORE_REL_MEASURED = 5.6e-14
SCORE_REL_TOL = 100 * SCORE_REL_MEASURED


@functools.lru_cache(maxsize=None)
def _integer_inputs():
    x, y = integer_rows(N_MAX)
    return x, y, as_f32(x).to(DEV), as_f32(y).to(DEV)


@functools.lru_cache(maxsize=None)
def _fold_ids(folds):
    return reference.fold_ids_cpu(N_MAX, folds, 42)


@functools.lru_cache(maxsize=None)
def _datagen_rows(n):
    y, X = ops.datagen(n, 30, 7, device=DEV)
    return X, y


@pytest.mark.parametrize("folds", [2, 3, 5])
@pytest.mark.parametrize("n", SIZES)
def test_fold_stats_exact_integer_sums(n, folds):
    x, y, xd, yd = _integer_inputs()
    got = ops.poly_fold_stats(xd[:n], yd[:n], folds=folds, seed=42, mu=0.0,
                              s=1.0)
    want = int64_fold_stats(x[:n], y[:n], folds, ids=_fold_ids(folds)[:n])
    assert got.dtype == torch.float64 and tuple(got.shape) == (folds, 18)
    assert np.array_equal(got.cpu().numpy(), want.astype(np.float64))


def test_repeatable_bitwise():
    X, y = _datagen_rows(2 * SWEEP + 5)
    a = ops.poly_fold_stats(X, y)
    b = ops.poly_fold_stats(X, y)
    assert torch.equal(a, b)


def test_offset_view_matches_fresh_copy():
    X, y = _datagen_rows(4099)
    Xv, yv = X[1:], y[1:]
    assert Xv.data_ptr() % 16 != 0
    got = ops.poly_fold_stats(Xv, yv)
    want = ops.poly_fold_stats(Xv.clone(), yv.clone())
    assert torch.equal(got, want)


@pytest.mark.parametrize("n", [4099, 2 * SWEEP + 5])
def test_real_rows_match_cpu_oracle(n):
    X, y = _datagen_rows(n)
    got = ops.poly_fold_stats(X, y).cpu().numpy()
    want = reference.poly_fold_stats_cpu(X.cpu(), y.cpu(), 5, 42, 50.0,
                                         50.0).numpy()
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-6)
    counts = np.bincount(reference.fold_ids_cpu(X.numel(), 5, 42),
                         minlength=5)
    assert np.array_equal(got[:, 0], counts)


def test_no_rows_gives_zeros():
    e = torch.empty(0, device=DEV)
    out = ops.poly_fold_stats(e, e, folds=3)
    assert tuple(out.shape) == (3, 18) and out.dtype == torch.float64
    assert out.device.type == "cuda" and not out.any()


def test_fold_count_checked_by_the_op():
    X, y = _datagen_rows(4099)
    core = ops._core(X.device)
    for folds in (1, 6):
        with pytest.raises(RuntimeError, match="folds"):
            core.poly_fold_stats(X, y, folds, 42, 50.0, 50.0)


@pytest.mark.parametrize("nblocks,K", [(1, 90), (257, 90), (1024, 90),
                                       (1024, 36), (300, 7)])
def test_wide_finalise_gives_the_one_block_bits(nblocks, K):
    g = torch.Generator(device="cpu").manual_seed(nblocks * 131 + K)
    ws = (torch.randn(nblocks, K, generator=g, dtype=torch.float64)
          * 1e6).to(DEV)
    core = ops._core(ws.device)
    narrow = core.reduce_finalize(ws, False)
    wide = core.reduce_finalize(ws, True)
    assert torch.equal(narrow, wide)
    np.testing.assert_allclose(wide.cpu().numpy(), ws.cpu().numpy().sum(0),
                               rtol=1e-12, atol=1e-6)


def test_device_selection_matches_cpu_path():
    X, y = quadratic_rows()
    cpu = GPUPolyRegressorCV().fit(X, y)
    dev = GPUPolyRegressorCV(device=DEV).fit(X.to(DEV), y.to(DEV))
    assert dev.best_params_ == cpu.best_params_
    assert dev.degree == 2
    a = np.asarray(dev.cv_results_["mean_test_mse"])
    b = np.asarray(cpu.cv_results_["mean_test_mse"])
    rel = np.abs(a - b) / b
    print("worst rel. deviation of device CV scores from CPU:", rel.max())
    assert rel.max() <= SCORE_REL_TOL
    pred = dev.predict(as_f32([50.0, 100.0]).to(DEV)).cpu().numpy()
    np.testing.assert_allclose(pred, [3.0, 1.0], atol=0.1)


def test_two_polycv_cycles_end_to_end(tmp_store):
    from bodywork_mlops_demo_amd.pipeline.cycle import CycleState, run_cycle
    from bodywork_mlops_demo_amd.store import contract

    state = CycleState(DEV, date(2026, 1, 1))
    cache: dict = {}
    for _ in range(2):
        day = state.date
        cap: dict = {}
        r = run_cycle(state, tmp_store, n_rows=4099, model_type="polycv",
                      scorer_cache=cache, capture=cap)
        state.drain_io()
        assert np.isfinite(r["online"]["MAPE"])
        assert np.isfinite(r["offline"]["MAPE"])
        trained = cap["model"]
        assert isinstance(trained, GPUPolyRegressorCV)
        rec = tmp_store.get_metrics_csv(contract.model_metrics_key(day))
        assert int(rec["cv_degree"]) == trained.degree
        assert float(rec["cv_l2"]) == trained.l2
        # what serving scored day t+1 with is the model that was trained:
        # the artefact round trip moves coefficients by ~1e-9 relative and
        # both sides evaluate the same fp32 Horner scheme, so a one-ulp
        # flip of an fp32 coefficient (<= 6e-8 * |coef|) is all that can
        # separate them
        want = trained.predict(cap["X"])
        torch.testing.assert_close(cap["scores"].to(want.device).float(),
                                   want, rtol=1e-5, atol=1e-4)
    assert state.cycle_count == 2
