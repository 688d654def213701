"""drift_histograms on the GPU: exact int64 equality with the numpy oracle
over sizes, bin counts, input kinds and misaligned views, plus one cycle
with a monitor end to end."""
from datetime import date

import numpy as np
import pytest
import torch

from bodywork_mlops_demo_amd import ops
from bodywork_mlops_demo_amd.ops import reference

pytestmark = pytest.mark.gpu

GRID_CAP = 1024          # DH_GRID_CAP of ops/hip/drift_hist.hip
SWEEP = GRID_CAP * 1024  # rows one sweep of the capped grid covers
SIZES = [0, 1, 3, 4, 5, 255, 256, 257, 1023, 4099]
BINS = [1, 16, 64, 256]
KINDS = ["uniform", "equal", "edges", "specials"]
N_BASE = SWEEP + 4099 + 3


def _spec(bins):
    from bodywork_mlops_demo_amd.monitoring.drift import HistSpec

    return HistSpec(bins=bins, x=(0, 64), label=(0, 64), score=(-8, 56),
                    residual=(-16, 16))


@pytest.fixture(scope="module")
def base():
    """Host arrays of every input kind, made once; tests slice them."""
    rng = np.random.default_rng(20261021)
    out = {}
    out["uniform"] = tuple(
        rng.uniform(-10, 74, N_BASE).astype(np.float32) for _ in range(3))
    out["equal"] = tuple(
        np.full(N_BASE, v, dtype=np.float32) for v in (32.0, 20.5, 19.25))
    # exact bin edges for every bin count in BINS (multiples of 1/4), the
    # range ends included
    out["edges"] = tuple(
        (rng.integers(-8, 264, N_BASE) * 0.25).astype(np.float32)
        for _ in range(3))
    sp = []
    for _ in range(3):
        v = rng.uniform(-10, 74, N_BASE).astype(np.float32)
        pick = rng.integers(0, 16, N_BASE)
        v[pick == 0] = np.nan
        v[pick == 1] = np.inf
        v[pick == 2] = -np.inf
        sp.append(v)
    out["specials"] = tuple(sp)
    return out


def _gpu(arrs, lo, n):
    return tuple(torch.from_numpy(a[lo:lo + n]).cuda() for a in arrs)


def _check(dev, host, bins):
    spec = _spec(bins)
    n = host[0].shape[0]
    got = ops.drift_histograms(*dev, spec)
    assert got.is_cuda and got.dtype == torch.int64
    assert tuple(got.shape) == (4, bins + 3)
    want = reference.drift_histograms_cpu(*host, bins, *spec.bin_params())
    assert torch.equal(got.cpu(), want)
    assert (got.sum(dim=1) == n).all()
    again = ops.drift_histograms(*dev, spec)
    assert torch.equal(got, again)


@pytest.mark.parametrize("bins", BINS)
@pytest.mark.parametrize("n", SIZES)
def test_matches_oracle(base, n, bins):
    for kind in KINDS:
        host = tuple(a[7:7 + n] for a in base[kind])
        _check(_gpu(base[kind], 7, n), host, bins)


@pytest.mark.parametrize("n", [1, 5, 257, 4099])
def test_misaligned_views(base, n):
    """t[1:] / t[3:] views are contiguous but not 16-byte aligned."""
    for kind in ("uniform", "specials"):
        full = tuple(torch.from_numpy(a[:n + 3]).cuda() for a in base[kind])
        for offs in ((1, 1, 1), (1, 3, 0), (3, 0, 1)):
            dev = tuple(t[o:][:n] for t, o in zip(full, offs))
            assert any(t.data_ptr() % 16 for t in dev)
            host = tuple(a[o:o + n] for a, o in zip(base[kind], offs))
            _check(dev, host, 64)


@pytest.mark.parametrize("bins", BINS)
def test_second_sweep_of_the_grid(base, bins):
    """grid_cap * 1024 + 4099 rows: the grid-stride loop runs twice."""
    n = SWEEP + 4099
    for kind in ("uniform", "equal"):
        host = tuple(a[:n] for a in base[kind])
        _check(_gpu(base[kind], 0, n), host, bins)


def test_cycle_with_monitor_reproduces_from_captured_tensors():
    from bodywork_mlops_demo_amd.monitoring.drift import (
        METRIC_KEYS, DriftMonitor)
    from bodywork_mlops_demo_amd.pipeline.cycle import CycleState, run_cycle

    mon = DriftMonitor()
    state = CycleState("cuda:0", date(2026, 3, 1))
    cap: dict = {}
    r = run_cycle(state, None, n_rows=10_000, model_type="linear",
                  capture=cap, drift_monitor=mon)
    online = r["online"]
    assert [k for k in online if k in METRIC_KEYS] == list(METRIC_KEYS)

    lo, scale = mon.spec.bin_params()
    bins = mon.spec.bins
    day = state._day_sizes[0]
    X_day, y_day = state.X[:day], state.y[:day]
    ref = reference.drift_histograms_cpu(
        X_day, y_day, cap["model"].predict(X_day), bins, lo, scale).numpy()
    assert (mon.reference == ref).all()
    cur = reference.drift_histograms_cpu(
        cap["X"], cap["labels"], cap["scores"], bins, lo, scale).numpy()
    assert cur[0].sum() == r["timings"]["rows_scored"]
    want = mon.statistics(ref, cur)
    assert online["drifted"] == want["drifted"]
    for k in METRIC_KEYS[:-1]:
        assert online[k] == pytest.approx(want[k], rel=1e-12, abs=1e-12)
