"""Data-drift monitor on the CPU path: the histogram oracle's slot rule,
the PSI / KS / JS / quantile statistics against hand-computed vectors, the
monitor's decision on generator data, the ``ks`` retrain policy of
``run_loop`` and the collective (gloo, world=2) monitor."""
import math
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from bodywork_mlops_demo_amd import ops

# what a test-metrics CSV and an `online` dict hold without a monitor
BASE_HEADER = ["date", "MAPE", "r_squared", "max_residual",
               "mean_response_time", "response_time_kind"]
BASE_ONLINE = {"MAPE", "r_squared", "max_residual", "mean_response_time",
               "response_time_kind", "rows_per_sec"}
DRIFT_KEYS = ["psi_x", "psi_label", "psi_score", "psi_residual",
              "ks_residual", "ks_critical", "residual_q05", "residual_q50",
              "residual_q95", "drifted"]


def _drift():
    from bodywork_mlops_demo_amd.monitoring import drift

    return drift


def _spec(bins, lo=0.0, hi=64.0, residual=None):
    r = (lo, hi)
    return _drift().HistSpec(bins=bins, x=r, label=r, score=r,
                             residual=residual or r)


# -- the oracle --------------------------------------------------------------

@pytest.mark.parametrize("bins", [1, 16, 64, 256])
def test_oracle_matches_np_histogram_away_from_edges(bins):
    rng = np.random.default_rng(bins)
    n = 5000
    spec = _drift().HistSpec(bins=bins, x=(0, 100), label=(0, 128),
                             score=(0, 128), residual=(-50, 50))
    width = [100 / bins, 128 / bins, 128 / bins, 100 / bins]
    lo = [0.0, 0.0, 0.0, -50.0]

    def mid(k):
        # values at 0.2..0.8 of a cell: a rounding of t cannot move them
        cell = rng.integers(-2, bins + 2, n)
        return (lo[k] + (cell + rng.uniform(0.2, 0.8, n)) * width[k]
                ).astype(np.float32)

    x, lab = mid(0), mid(1)
    # residual = lab - score must sit mid-cell too: derive score from it
    res = mid(3)
    score = (lab - res).astype(np.float32)
    res = lab - score  # what the oracle will bin (fp32)
    frac = ((res.astype(np.float64) - lo[3]) / width[3]) % 1.0
    keep = (frac > 0.05) & (frac < 0.95)
    fs = ((score.astype(np.float64) - lo[2]) / width[2]) % 1.0
    keep &= (fs > 1e-3) & (fs < 1 - 1e-3)
    x, lab, score, res = x[keep], lab[keep], score[keep], res[keep]

    h = ops.drift_histograms(torch.from_numpy(x), torch.from_numpy(lab),
                             torch.from_numpy(score), spec).numpy()
    assert h.dtype == np.int64 and h.shape == (4, bins + 3)
    for k, (v, (a, b)) in enumerate(zip((x, lab, score, res), spec.ranges())):
        inner, _ = np.histogram(v.astype(np.float64), bins=bins, range=(a, b))
        # np.histogram closes the last bin on the right; no value sits there
        assert (h[k, 1:bins + 1] == inner).all()
        assert h[k, 0] == (v < a).sum()
        assert h[k, bins + 1] == (v >= b).sum()
        assert h[k, bins + 2] == 0
        assert h[k].sum() == v.shape[0]


def test_oracle_exact_edges_and_specials():
    bins = 64
    spec = _spec(bins)
    inf, nan = float("inf"), float("nan")
    #                 under  bin1  bin1  bin2  bin64 over  over under  nan
    x = torch.tensor([-1.0, 0.0, 0.5, 1.0, 63.0, 64.0, inf, -inf, nan,
                      -0.0, 63.999996, 1e30, -1e30])
    labels = torch.tensor([inf, inf, -inf, nan, 5.0, 3.0, 7.0, 0.0, 1.0,
                           2.0, 10.0, 10.0, 64.0])
    scores = torch.tensor([inf, -inf, -inf, 1.0, 5.0, 1.0, 7.0, 1.0, nan,
                           2.0, 9.5, 74.0, 0.0])
    h = ops.drift_histograms(x, labels, scores, spec).numpy()
    want_x = np.zeros(bins + 3, dtype=np.int64)
    for slot in (0, 1, 1, 2, 64, 65, 65, 0, 66, 1, 64, 65, 0):
        want_x[slot] += 1
    assert (h[0] == want_x).all()
    # residual row: inf-inf, inf+inf, -inf+inf, nan, 0, 2, 0, -1, nan, 0,
    # 0.5, -64, 64
    want_r = np.zeros(bins + 3, dtype=np.int64)
    for slot in (66, 65, 66, 66, 1, 3, 1, 0, 66, 1, 1, 0, 65):
        want_r[slot] += 1
    assert (h[3] == want_r).all()
    assert (h.sum(axis=1) == x.numel()).all()


def test_oracle_integer_inputs_fill_one_bin_each():
    spec = _spec(64)
    v = torch.arange(64, dtype=torch.float32)
    h = ops.drift_histograms(v, v, v, spec).numpy()
    for k in range(3):
        assert (h[k, 1:65] == 1).all() and h[k, 0] == h[k, 65] == 0
    assert h[3, 1] == 64  # residual 0 everywhere


@pytest.mark.parametrize("bins", [1, 256])
def test_oracle_bins_extremes_and_row_totals(bins):
    rng = np.random.default_rng(3)
    n = 4099
    v = [torch.from_numpy(rng.uniform(-10, 80, n).astype(np.float32))
         for _ in range(3)]
    h = ops.drift_histograms(*v, _spec(bins)).numpy()
    assert h.shape == (4, bins + 3)
    assert (h.sum(axis=1) == n).all()
    if bins == 1:
        x = v[0].numpy()
        assert h[0, 1] == ((x >= 0) & (x < 64)).sum()


def test_oracle_empty_input():
    e = torch.empty(0)
    h = ops.drift_histograms(e, e, e, _spec(16))
    assert h.shape == (4, 19) and int(h.sum()) == 0


def test_histspec_scale_is_fp32_and_validated():
    d = _drift()
    lo, scale = d.HistSpec(bins=64, residual=(-40, 40)).bin_params()
    assert lo == [0.0, 0.0, 0.0, -40.0]
    want = [np.float32(64) / np.float32(100), np.float32(0.5),
            np.float32(0.5), np.float32(0.8)]
    assert scale == [float(w) for w in want]
    with pytest.raises(ValueError):
        d.HistSpec(bins=0)
    with pytest.raises(ValueError):
        d.HistSpec(bins=257)
    with pytest.raises(ValueError):
        d.HistSpec(x=(1, 1))


# -- statistics on count vectors ---------------------------------------------

def test_psi_hand_computed_and_symmetric():
    d = _drift()
    a, b = [10, 30, 60], [20, 30, 50]
    # eps = 0.5, K = 3: p = (10.5, 30.5, 60.5)/101.5, q = (20.5, 30.5, 50.5)/101.5
    p = np.array([10.5, 30.5, 60.5]) / 101.5
    q = np.array([20.5, 30.5, 50.5]) / 101.5
    want = float(np.sum((q - p) * np.log(q / p)))
    assert d.psi(a, b) == pytest.approx(want, rel=1e-12)
    assert want == pytest.approx(0.08371, abs=1e-4)  # by hand
    assert d.psi(a, b) == pytest.approx(d.psi(b, a), rel=1e-12)
    assert d.psi(a, a) == 0.0
    # smoothing keeps an empty cell finite
    assert math.isfinite(d.psi([0, 10], [10, 0]))
    assert d.psi(a, b, eps=0.0) == pytest.approx(
        0.1 * math.log(2) - 0.1 * math.log(5 / 6), rel=1e-12)


def test_ks_hand_computed():
    d = _drift()
    # CDFs (0.1, 0.4, 1.0) vs (0.2, 0.5, 1.0)
    assert d.ks([10, 30, 60], [20, 30, 50]) == pytest.approx(0.1, abs=1e-15)
    # different sample sizes: (0.25, 1.0) vs (0.5, 1.0)
    assert d.ks([1, 3], [50, 50]) == pytest.approx(0.25, abs=1e-15)
    a = [3, 0, 7, 11, 2]
    assert d.ks(a, a) == 0.0
    assert d.ks([5, 0], [0, 5]) == 1.0


def test_js_hand_computed():
    d = _drift()
    assert d.js([5, 0], [0, 5]) == pytest.approx(math.log(2), rel=1e-12)
    assert d.js([4, 4], [1, 1]) == 0.0
    # p = (.5, .5), q = (.25, .75), m = (.375, .625)
    want = 0.5 * (0.5 * math.log(0.5 / 0.375) + 0.5 * math.log(0.5 / 0.625)) \
        + 0.5 * (0.25 * math.log(0.25 / 0.375) + 0.75 * math.log(0.75 / 0.625))
    assert d.js([2, 2], [1, 3]) == pytest.approx(want, rel=1e-12)
    assert d.js([2, 2], [1, 3]) == pytest.approx(d.js([1, 3], [2, 2]),
                                                 rel=1e-12)


def test_quantile_hand_computed():
    d = _drift()
    # [under, 4 bins over (0, 8), over]; width 2
    c = [0, 10, 10, 10, 10, 0]
    assert d.quantile(c, (0, 8), 0.5) == pytest.approx(4.0)
    assert d.quantile(c, (0, 8), 0.25) == pytest.approx(2.0)
    assert d.quantile(c, (0, 8), 0.125) == pytest.approx(1.0)
    assert d.quantile(c, (0, 8), 0.95) == pytest.approx(7.6)
    # 10 % below the range: the 5 % quantile is the lower edge
    c = [10, 40, 0, 0, 40, 10]
    assert d.quantile(c, (0, 8), 0.05) == 0.0
    assert d.quantile(c, (0, 8), 0.97) == 8.0
    # target 30 of 100: 20 into the first bin's 40 -> 0 + 0.5 * 2
    assert d.quantile(c, (0, 8), 0.30) == pytest.approx(1.0)
    assert math.isnan(d.quantile([0, 0, 0], (0, 1), 0.5))


def test_ks_critical_formula():
    d = _drift()
    want = math.sqrt(-math.log(0.0005) / 2) * math.sqrt(2e5 / 1e10)
    assert d.ks_critical(100_000, 100_000) == pytest.approx(want, rel=1e-12)
    assert want == pytest.approx(0.0087, abs=5e-5)
    # the reference's day size: far above the generator's largest KS (~0.02)
    assert d.ks_critical(1440, 1440) == pytest.approx(0.0727, abs=5e-5)
    assert d.ks_critical(1000, 4000, alpha=0.05) == pytest.approx(
        1.3581 * math.sqrt(5000 / 4e6), rel=1e-4)


# -- the monitor's decision on generator data --------------------------------

@pytest.fixture(scope="module")
def day1_fit():
    n = 100_000
    y, X = ops.datagen(n, 1, 123)
    a, b = ops.solve_ols(ops.linreg_stats(X, y))
    return X, y, a, b


@pytest.mark.parametrize("bins", [16, 64])
def test_monitor_decision_follows_the_generators_drift(day1_fit, bins):
    d = _drift()
    X, y, a, b = day1_fit
    mon = d.DriftMonitor(d.HistSpec(bins=bins, residual=(-40, 40)))
    with pytest.raises(RuntimeError):
        mon.observe(X, y, X)
    mon.set_reference(X, y, ops.linear_score(X, a, b))
    out = {}
    for day in (1, 8, 16):
        y2, X2 = ops.datagen(100_000, day, 456)
        out[day] = mon.observe(X2, y2, ops.linear_score(X2, a, b))
        assert list(out[day]) == DRIFT_KEYS
    crit = out[1]["ks_critical"]
    # ~93.7k rows a day survive the y >= 0 cull
    assert crit == pytest.approx(0.0090, abs=2e-4)
    assert out[1]["ks_residual"] < 0.5 * crit and not out[1]["drifted"]
    assert out[8]["ks_residual"] > crit and out[8]["drifted"]
    assert out[16]["ks_residual"] > out[8]["ks_residual"]
    assert out[16]["drifted"]
    assert 0.015 < out[16]["ks_residual"] < 0.022
    # a floor above the observed distance overrides the critical value
    floor = d.DriftMonitor(mon.spec, ks_threshold=0.05)
    floor.reference = mon.reference
    y2, X2 = ops.datagen(100_000, 16, 456)
    assert not floor.observe(X2, y2, ops.linear_score(X2, a, b))["drifted"]


def test_monitor_statistics_use_all_ordinary_cells():
    d = _drift()
    mon = d.DriftMonitor(d.HistSpec(bins=2, residual=(0, 2)))
    ref = np.zeros((4, 5), dtype=np.int64)
    cur = np.zeros((4, 5), dtype=np.int64)
    ref[:] = [10, 40, 40, 10, 0]
    cur[:] = [30, 30, 30, 10, 7]   # mass moved into the under cell + 7 NaN
    s = mon.statistics(ref, cur)
    assert s["ks_residual"] == pytest.approx(0.2)  # at the under cell
    # NaN rows are outside the ordered sample
    assert s["ks_critical"] == pytest.approx(d.ks_critical(100, 100))
    assert s["psi_residual"] == pytest.approx(d.psi(ref[3], cur[3]))
    assert s["residual_q50"] == pytest.approx(0.0 + (20 / 30) * 1.0)


# -- run_loop -----------------------------------------------------------------

def _csv_rows(store):
    from bodywork_mlops_demo_amd.store import contract

    rows = []
    for key, _ in store.all_by_date(contract.TEST_METRICS_PREFIX):
        text = store.get_bytes(key).decode().strip().splitlines()
        rows.append((text[0].split(","), text[1].split(",")))
    return rows


def test_run_loop_ks_policy_carries_the_drift_columns(tmp_store):
    from bodywork_mlops_demo_amd.pipeline.loop import run_loop

    results = run_loop(tmp_store, days=3, n_rows=1440, device="cpu",
                       retrain_policy="ks")
    assert len(results) == 3
    for r in results:
        assert set(r["online"]) == BASE_ONLINE | set(DRIFT_KEYS)
        assert isinstance(r["online"]["drifted"], bool)
        # one day of 1440 rows cannot resolve this drift: critical value
        # ~0.073-0.075 against a largest KS of ~0.02 plus sampling noise
        assert r["online"]["ks_critical"] > 0.07
    assert results[0]["timings"]["train_s"] > 0
    for prev, r in zip(results, results[1:]):
        assert (r["timings"]["train_s"] > 0) == prev["online"]["drifted"]
    rows = _csv_rows(tmp_store)
    assert len(rows) == 3
    for (header, vals), r in zip(rows, results):
        assert header == BASE_HEADER + DRIFT_KEYS
        rec = dict(zip(header, vals))
        assert float(rec["ks_residual"]) == r["online"]["ks_residual"]
        assert rec["drifted"] == str(int(r["online"]["drifted"]))


def test_run_loop_monitor_flag_leaves_the_policy_alone(tmp_store):
    from bodywork_mlops_demo_amd.pipeline.loop import run_loop

    results = run_loop(tmp_store, days=2, n_rows=1440, device="cpu",
                       drift_monitor=True)
    assert all(r["timings"]["train_s"] > 0 for r in results)  # "always"
    assert all("ks_residual" in r["online"] for r in results)

    from bodywork_mlops_demo_amd.monitoring.analytics import drift_report

    summary = drift_report(tmp_store)["summary"]
    assert summary["days_drifted"] == sum(
        r["online"]["drifted"] for r in results[:summary["days"]])
    assert summary["max_ks_residual"] >= summary["mean_ks_residual"] > 0


def test_run_loop_defaults_are_unchanged(tmp_store):
    """Guard: passes with and without the feature."""
    from bodywork_mlops_demo_amd.pipeline.loop import run_loop

    results = run_loop(tmp_store, days=3, n_rows=1440, device="cpu")
    for r in results:
        assert set(r["online"]) == BASE_ONLINE
    for header, vals in _csv_rows(tmp_store):
        assert header == BASE_HEADER
        assert len(vals) == len(BASE_HEADER)


# -- collective monitor --------------------------------------------------------

def _shards(world):
    n = 6000
    y, X = ops.datagen(n, 1, 11)
    y2, X2 = ops.datagen(n, 16, 12)
    a, b = 1.0, 0.5
    cut = lambda t, r: t[r::world].clone()  # noqa: E731
    return (X, y, ops.linear_score(X, a, b)), \
        (X2, y2, ops.linear_score(X2, a, b)), cut


def _monitor_worker(rank, world, port, out):
    os.environ.update(
        RANK=str(rank), WORLD_SIZE=str(world),
        MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), LOCAL_RANK=str(rank),
    )
    import torch.distributed as dist

    from bodywork_mlops_demo_amd.monitoring.drift import DriftMonitor
    from bodywork_mlops_demo_amd.parallel import init_distributed

    init_distributed(backend="gloo")
    ref, cur, cut = _shards(world)
    mon = DriftMonitor(process_group=dist.group.WORLD)
    mon.set_reference(*(cut(t, rank) for t in ref))
    out[rank] = mon.observe(*(cut(t, rank) for t in cur))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(120)
def test_dp_monitor_is_collective_and_matches_single_process():
    ctx = mp.get_context("spawn")
    with ctx.Manager() as mgr:
        out = mgr.dict()
        mp.spawn(_monitor_worker, args=(2, 29653, out), nprocs=2, join=True)
        results = dict(out)
    assert results[0] == results[1]

    from bodywork_mlops_demo_amd.monitoring.drift import DriftMonitor

    ref, cur, _ = _shards(2)
    mon = DriftMonitor()
    mon.set_reference(*ref)
    assert mon.observe(*cur) == results[0]
