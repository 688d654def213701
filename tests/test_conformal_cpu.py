"""Conformal prediction intervals on the CPU path: the numpy oracles, the
statistical validity of the calibration, the artefact round trip, stage 1,
the service wire, stage 4, the loop and the two-rank select."""
import io
import math
import os
from datetime import date

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from bodywork_mlops_demo_amd import ops
from bodywork_mlops_demo_amd.models import (
    Calibration,
    GPULinearRegressor,
    GPUMLPRegressor,
    GPUPolyRegressor,
    regressor_from_artifact,
)
from bodywork_mlops_demo_amd.ops import reference
from bodywork_mlops_demo_amd.stages import datagen, loadtest, train
from bodywork_mlops_demo_amd.store import contract


# -- oracles -----------------------------------------------------------------

def _direct(labels, scores, levels):
    """The definition, written out with Python lists."""
    r = [abs(np.float32(np.float32(a) - np.float32(b)))
         for a, b in zip(labels, scores)]
    v = sorted(x for x in r if not math.isnan(x))
    m = len(v)
    out = []
    for L in levels:
        k = math.ceil((m + 1) * L)
        out.append(np.float32(np.inf) if k > m else v[k - 1])
    return np.float32(out), m, len(r) - m


@pytest.mark.parametrize("kind", ["random", "ties", "specials"])
@pytest.mark.parametrize("n", [0, 1, 2, 9, 10, 19, 20, 257])
def test_oracle_against_a_direct_sort(kind, n):
    rng = np.random.default_rng(n + 1)
    lab = rng.normal(50, 20, n).astype(np.float32)
    sc = rng.normal(50, 20, n).astype(np.float32)
    if kind == "ties":
        lab = rng.integers(0, 4, n).astype(np.float32)
        sc = np.zeros(n, dtype=np.float32)
    if kind == "specials" and n:
        lab[::3] = np.nan
        sc[1::5] = np.inf
        lab[1::10] = np.inf  # inf - inf
    levels = (0.5, 0.8, 0.9, 0.99)
    with np.errstate(invalid="ignore"):
        want, m, n_nan = _direct(lab, sc, levels)
    hw, gm, gn = ops.residual_quantiles(torch.from_numpy(lab),
                                        torch.from_numpy(sc), levels)
    assert hw.dtype == torch.float32 and (gm, gn) == (m, n_nan)
    assert np.array_equal(hw.numpy().view(np.int32), want.view(np.int32))


def test_rank_formula():
    assert {m: reference.conformal_rank(m, 0.9) for m in (0, 1, 9, 10, 19)} \
        == {0: 1, 1: 2, 9: 9, 10: 10, 19: 18}
    r = np.arange(1, 20, dtype=np.float32)          # m = 19: rank 18
    assert reference.select_residuals_cpu(r, (0.9,))[0].item() == 18.0
    for m in (0, 1):                                 # rank above m: +inf
        hw, gm, _ = reference.select_residuals_cpu(r[:m], (0.9,))
        assert gm == m and math.isinf(hw.item())
    assert reference.select_residuals_cpu(r[:9], (0.9,))[0].item() == 9.0
    assert reference.select_residuals_cpu(r[:10], (0.9,))[0].item() == 10.0


def test_levels_are_checked():
    y = torch.zeros(4)
    for bad in ((), (0.0,), (1.0,), (0.1, 0.2, 0.3, 0.4, 0.5)):
        with pytest.raises(ValueError):
            ops.residual_quantiles(y, y, bad)


def test_coverage_oracle():
    lab = np.float32([0, 1, 2, 3, np.nan, np.inf, 5])
    sc = np.float32([0, 0, 0, 0, 0, 0, np.inf])
    got = ops.interval_coverage(torch.from_numpy(sc), torch.from_numpy(lab),
                                [2.0, np.inf])
    # |r| = 0 1 2 3 nan inf inf; -1 padding counts nothing
    assert got.tolist() == [7.0, 3.0, 6.0, 0.0, 0.0]
    assert got.dtype == torch.float64


def test_split_linear_is_the_plain_select_on_the_split():
    y, X = ops.datagen(3000, 12, 5)
    got = ops.linear_split_residual_quantiles(X, y, (1.0, 0.5), (0.9, 0.95))
    _, _, X_te, y_te = ops.random_split(X, y, 0.2, seed=42)
    want = ops.residual_quantiles(y_te, ops.linear_score(X_te, 1.0, 0.5),
                                  (0.9, 0.95))
    assert torch.equal(got[0], want[0]) and got[1:] == want[1:]
    assert got[1] == y_te.numel()


# -- statistical validity ----------------------------------------------------

def test_calibrated_band_covers_a_fresh_draw():
    """Calibrate at 0.9 on one draw of a day, check a fresh draw of the same
    day.  The fresh coverage is binomial(n, c) around the band's true
    coverage c, and c itself is within sqrt(0.09 / m) ~ 0.0015 of 0.9 for
    the m ~ 40k calibration rows here — small beside the fresh draw's
    sqrt(0.09 / n) ~ 0.0042 at n ~ 5k, so the 1e-3 band of stage 4 (z =
    3.09, here on both sides) is the bound."""
    y, X = ops.datagen(200_000, 100, seed=11)
    model = GPULinearRegressor()
    model.fit_split(X, y, 0.2, seed=42)
    hw, m, n_nan = ops.linear_split_residual_quantiles(
        X, y, (model.intercept_, model.coef_), (0.9,))
    assert n_nan == 0 and 36_000 < m < 40_000
    cal = Calibration.from_select((0.9,), (hw, m, n_nan))
    y2, X2 = ops.datagen(5_500, 100, seed=12)
    out = loadtest.coverage_metrics(cal, model.predict(X2), y2)
    n = y2.numel()
    half = loadtest.COVERAGE_Z * math.sqrt(0.9 * 0.1 / n)
    print("coverage", out["pi90_coverage"], "band", 0.9 - half, 0.9 + half)
    assert 0.9 - half <= out["pi90_coverage"] <= 0.9 + half
    assert out["pi90_ok"] == 1
    assert out["pi90_halfwidth"] == cal.halfwidths[0]
    # sigma = 10: the 90 % band of a normal residual is 1.645 sigma; the
    # y >= 0 cull takes away under a tenth of the rows, all from one tail,
    # which narrows the band but not below the normal 80 % band (1.28 sigma)
    assert 12.8 < cal.halfwidths[0] < 16.45 * 1.02


def test_coverage_gate_trips_on_a_band_that_is_too_narrow():
    y, X = ops.datagen(5_000, 100, seed=13)
    cal = Calibration((0.9,), (10.0,), m=1000)   # ~68 % of sigma = 10
    out = loadtest.coverage_metrics(cal, 1.0 + 0.5 * X, y)
    assert out["pi90_ok"] == 0 and 0.6 < out["pi90_coverage"] < 0.75


# -- the Calibration value and the artefact ----------------------------------

CAL = Calibration((0.9, 0.95), (15.5, 19.25), m=1234, n_nan=2,
                  date=date(2026, 1, 3))


def test_calibration_value():
    assert CAL.halfwidth(0.95) == 19.25 and CAL.date == "2026-01-03"
    with pytest.raises(ValueError, match="0.9, 0.95"):
        CAL.halfwidth(0.8)
    d = CAL.as_dict()
    assert type(d) is dict and Calibration.from_dict(d) == CAL
    assert {type(v) for v in d["halfwidths"]} == {float}


def _models():
    lin = GPULinearRegressor(1.0, 0.5)
    poly = GPUPolyRegressor(degree=2)
    poly.coef_t_ = [26.0, 25.0, 0.5]
    mlp = GPUMLPRegressor(hidden=32, seed=3)
    return {"linear": lin, "poly": poly, "mlp": mlp}


@pytest.mark.parametrize("kind", ["linear", "poly", "mlp"])
def test_artefact_round_trip(kind):
    import joblib

    model = _models()[kind]
    X = np.linspace(0, 100, 17).reshape(-1, 1)
    plain = model.to_sklearn()
    assert not hasattr(plain, "conformal_")
    model.conformal_ = CAL
    bio = io.BytesIO()
    joblib.dump(model.to_sklearn(), bio)
    bio.seek(0)
    sk = joblib.load(bio)
    assert type(sk.conformal_) is dict and sk.conformal_ == CAL.as_dict()
    assert np.array_equal(sk.predict(X), plain.predict(X))
    back = regressor_from_artifact(sk)
    assert back.conformal_ == CAL
    assert regressor_from_artifact(plain).conformal_ is None
    # hot redeploy carries it, in both directions
    target = regressor_from_artifact(plain)
    assert target.copy_weights_from(back) and target.conformal_ == CAL
    assert target.copy_weights_from(regressor_from_artifact(plain))
    assert target.conformal_ is None


# -- stage 1 -----------------------------------------------------------------

@pytest.fixture()
def seeded_store(tmp_store):
    for day in (1, 2, 3):
        datagen.run(tmp_store, n=500, date=date(2026, 1, day), device="cpu",
                    seed=day)
    return tmp_store


BASE_HEADER = ["date", "MAPE", "r_squared", "max_residual"]


@pytest.mark.parametrize("model_type", ["linear", "poly2", "polycv2"])
def test_stage1_columns(seeded_store, model_type):
    key = contract.model_metrics_key(date(2026, 1, 3))
    plain = train.run(seeded_store, model_type=model_type, device="cpu")
    before = seeded_store.get_bytes(key)
    assert not hasattr(seeded_store.get_latest_model()[0], "conformal_")
    metrics, model = train.run(seeded_store, model_type=model_type,
                               device="cpu", conformal_levels=(0.9, 0.975),
                               return_model=True)
    assert metrics == plain
    rec = seeded_store.get_metrics_csv(key)
    cv = (["cv_degree", "cv_l2", "cv_mse", "cv_folds"]
          if model_type.startswith("polycv") else [])
    assert list(rec) == BASE_HEADER + cv + [
        "pi_cal_n", "pi90_halfwidth", "pi97.5_halfwidth"]
    cal = model.conformal_
    assert cal.levels == (0.9, 0.975) and cal.date == "2026-01-03"
    assert int(rec["pi_cal_n"]) == cal.m
    assert float(rec["pi90_halfwidth"]) == cal.halfwidths[0]
    assert float(rec["pi97.5_halfwidth"]) == cal.halfwidths[1]
    assert 10 < cal.halfwidths[0] < cal.halfwidths[1] < 40
    # the hold-out is the philox 20 %
    y_np, X_np, _ = seeded_store.get_all_datasets()
    _, _, X_te, y_te = ops.random_split(torch.from_numpy(X_np),
                                        torch.from_numpy(y_np), 0.2, seed=42)
    want = ops.residual_quantiles(y_te, model.predict(X_te), cal.levels)
    assert cal.m == want[1] == y_te.numel()
    assert list(cal.halfwidths) == want[0].tolist()
    art = seeded_store.get_latest_model()[0]
    assert art.conformal_ == cal.as_dict()
    # and without levels the record is what it was
    train.run(seeded_store, model_type=model_type, device="cpu")
    assert seeded_store.get_bytes(key) == before
    assert list(seeded_store.get_metrics_csv(key)) == BASE_HEADER + cv


def test_stage1_cli_levels():
    assert train.parse_levels("0.9,0.95") == (0.9, 0.95)
    import argparse

    for bad in ("1.5", "0.1,0.2,0.3,0.4,0.5", ""):
        with pytest.raises(argparse.ArgumentTypeError):
            train.parse_levels(bad)


# -- the service -------------------------------------------------------------

def test_service_intervals(seeded_store):
    from fastapi.testclient import TestClient

    from bodywork_mlops_demo_amd.serving.server import create_app

    _, model = train.run(seeded_store, model_type="linear", device="cpu",
                         conformal_levels=(0.9, 0.95), return_model=True)
    h90, h95 = model.conformal_.halfwidths
    with TestClient(create_app(seeded_store, device="cpu")) as client:
        plain = client.post("/score/v1", json={"X": 50}).json()
        assert set(plain) == {"prediction", "model_info"}
        r = client.post("/score/v1", json={"X": 50, "confidence": 0.9})
        body = r.json()
        assert r.status_code == 200
        assert set(body) == {"prediction", "model_info", "interval",
                             "confidence"}
        p = body["prediction"]
        assert p == plain["prediction"] and body["confidence"] == 0.9
        assert body["interval"] == [p - h90, p + h90]

        body = client.post("/score/v1", json={"X": [10.0, 20.0],
                                              "confidence": 0.95}).json()
        assert body["interval"] == [[q - h95, q + h95]
                                    for q in body["prediction"]]
        body = client.post("/score/v1/batch",
                           json={"X": [1.0, 2.0, 3.0],
                                 "confidence": 0.9}).json()
        assert set(body) == {"predictions", "n", "model_info", "interval",
                             "confidence"}
        assert body["interval"] == [[q - h90, q + h90]
                                    for q in body["predictions"]]
        assert set(client.post("/score/v1/batch",
                               json={"X": [1.0]}).json()) == {
            "predictions", "n", "model_info"}

        for path, x in (("/score/v1", 50), ("/score/v1/batch", [50])):
            r = client.post(path, json={"X": x, "confidence": 0.8})
            assert r.status_code == 422
            assert "0.9, 0.95" in r.json()["detail"]

        X = np.float32([10.0, 20.0, 30.0])
        r = client.post("/score/v1/binary", content=X.tobytes(),
                        headers={"Content-Type": "application/octet-stream"})
        assert r.headers["X-Interval-Levels"] == "0.9,0.95"
        assert [float(v) for v in
                r.headers["X-Interval-Halfwidths"].split(",")] == [h90, h95]
        assert client.get("/healthz").json()["interval_levels"] == [0.9, 0.95]

        # a retrain on one more day, then a reload: the new half-width
        datagen.run(seeded_store, n=500, date=date(2026, 1, 4), device="cpu",
                    seed=4)
        _, model2 = train.run(seeded_store, model_type="linear",
                              device="cpu", conformal_levels=(0.9,),
                              return_model=True)
        new = model2.conformal_.halfwidths[0]
        assert new != h90
        r = client.post("/reload/v1")
        assert r.json()["interval_levels"] == [0.9]
        body = client.post("/score/v1", json={"X": 50,
                                              "confidence": 0.9}).json()
        p = body["prediction"]
        assert body["interval"] == [p - new, p + new]
        assert client.post("/score/v1", json={
            "X": 50, "confidence": 0.95}).status_code == 422


def test_service_without_calibration_is_unchanged(seeded_store):
    from fastapi.testclient import TestClient

    from bodywork_mlops_demo_amd.serving.server import create_app

    train.run(seeded_store, model_type="linear", device="cpu")
    with TestClient(create_app(seeded_store, device="cpu")) as client:
        r = client.post("/score/v1", json={"X": 50, "confidence": 0.9})
        assert r.status_code == 422 and "none" in r.json()["detail"]
        assert set(client.post("/score/v1", json={"X": 50}).json()) == {
            "prediction", "model_info"}
        assert set(client.get("/healthz").json()) == {
            "status", "model_date", "model_info"}
        assert set(client.post("/reload/v1").json()) == {
            "status", "model_date", "model_info"}
        X = np.float32([10.0])
        r = client.post("/score/v1/binary", content=X.tobytes())
        assert not [h for h in r.headers if h.lower().startswith("x-interval")]


# -- stage 4 and the loop ----------------------------------------------------

TEST_HEADER = ["date", "MAPE", "r_squared", "max_residual",
               "mean_response_time", "response_time_kind"]
PI = ["pi90_coverage", "pi90_halfwidth", "pi90_ok"]


def test_stage4_columns_come_last(seeded_store):
    from bodywork_mlops_demo_amd.monitoring.drift import (
        METRIC_KEYS,
        DriftMonitor,
    )
    from bodywork_mlops_demo_amd.serving.scorer import BatchedScorer

    _, model = train.run(seeded_store, model_type="linear", device="cpu",
                         conformal_levels=(0.9,), return_model=True)
    scorer = BatchedScorer(model, "cpu")
    key = contract.test_metrics_key(date(2026, 1, 3))
    loadtest.run(seeded_store, device="cpu", scorer=scorer)
    assert list(seeded_store.get_metrics_csv(key)) == TEST_HEADER

    # True: the calibration comes from the latest artefact
    m = loadtest.run(seeded_store, device="cpu", scorer=scorer,
                     conformal=True)
    rec = seeded_store.get_metrics_csv(key)
    assert list(rec) == TEST_HEADER + PI
    assert float(rec["pi90_coverage"]) == m["pi90_coverage"]
    assert float(rec["pi90_halfwidth"]) == model.conformal_.halfwidths[0]
    assert rec["pi90_ok"] in (0, 1, "0", "1")
    y_np, X_np = seeded_store.get_dataset(
        contract.dataset_key(date(2026, 1, 3)))
    inside = np.abs(y_np.astype(np.float32)
                    - model.predict(torch.from_numpy(X_np)).numpy()) \
        <= np.float32(model.conformal_.halfwidths[0])
    assert m["pi90_coverage"] == inside.mean()

    mon = DriftMonitor()
    X, y = torch.from_numpy(X_np), torch.from_numpy(y_np)
    mon.set_reference(X, y, model.predict(X))
    loadtest.run(seeded_store, device="cpu", scorer=scorer,
                 drift_monitor=mon, conformal=model.conformal_)
    assert list(seeded_store.get_metrics_csv(key)) == \
        TEST_HEADER + list(METRIC_KEYS) + PI

    train.run(seeded_store, model_type="linear", device="cpu")
    with pytest.raises(ValueError, match="no conformal calibration"):
        loadtest.run(seeded_store, device="cpu", scorer=scorer,
                     conformal=True)


def test_loop_fills_the_columns(tmp_store):
    from bodywork_mlops_demo_amd.monitoring.analytics import drift_report
    from bodywork_mlops_demo_amd.pipeline.loop import run_loop

    res = run_loop(tmp_store, days=3, n_rows=1500, device="cpu",
                   start_date="2026-02-01", conformal_levels=(0.9,))
    assert len(res) == 3
    for i, r in enumerate(res):
        on, cal = r["online"], r["offline"]["conformal"]
        assert list(on)[-3:] == PI
        assert on["pi90_halfwidth"] == cal.halfwidths[0]
        assert 0.8 < on["pi90_coverage"] < 1.0 and on["pi90_ok"] in (0, 1)
        d = date(2026, 2, 2 + i)
        rec = tmp_store.get_metrics_csv(contract.test_metrics_key(d))
        assert list(rec) == TEST_HEADER + PI
        rec = tmp_store.get_metrics_csv(
            contract.model_metrics_key(date(2026, 2, 1 + i)))
        assert list(rec) == BASE_HEADER + ["pi_cal_n", "pi90_halfwidth"]
    rep = drift_report(tmp_store)
    # pandas' float parser is within an ulp or so, not exact
    assert [c for _, c in rep["coverage"]["90"]["per_day"]] == pytest.approx(
        [r["online"]["pi90_coverage"] for r in res], rel=1e-12)
    assert "pi90_mean_coverage" in rep["summary"]

    plain = run_loop(None, days=1, n_rows=1500, device="cpu",
                     start_date="2026-02-01")
    assert not [k for k in plain[0]["online"] if k.startswith("pi")]
    assert "conformal" not in plain[0]["offline"]


# -- two ranks ---------------------------------------------------------------

def _toy(n=4001, seed=3):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 100, n).astype(np.float32)
    y = (1.0 + 0.5 * X + rng.normal(0, 10, n)).astype(np.float32)
    y[::97] = np.nan
    return X, y


LEVELS = (0.5, 0.9, 0.99)


def _select_worker(rank, world, port, out):
    os.environ.update(
        RANK=str(rank), WORLD_SIZE=str(world),
        MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), LOCAL_RANK=str(rank),
    )
    import torch.distributed as dist

    from bodywork_mlops_demo_amd.parallel import init_distributed

    init_distributed(backend="gloo")
    X, y = _toy()
    Xs = torch.from_numpy(X[rank::world].copy())
    ys = torch.from_numpy(y[rank::world].copy())
    hw, m, n_nan = ops.residual_quantiles(ys, 1.0 + 0.5 * Xs, LEVELS,
                                          process_group=dist.group.WORLD)
    cal = Calibration.from_select(LEVELS, (hw, m, n_nan))
    cov = loadtest.coverage_metrics(cal, 1.0 + 0.5 * Xs, ys,
                                    process_group=dist.group.WORLD)
    out[rank] = (hw.tolist(), m, n_nan, cov)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(120)
def test_two_ranks_select_the_quantiles_of_the_union():
    ctx = mp.get_context("spawn")
    with ctx.Manager() as mgr:
        out = mgr.dict()
        mp.spawn(_select_worker, args=(2, 29651, out), nprocs=2, join=True)
        results = dict(out)
    assert results[0] == results[1]
    X, y = _toy()
    Xt, yt = torch.from_numpy(X), torch.from_numpy(y)
    hw, m, n_nan = ops.residual_quantiles(yt, 1.0 + 0.5 * Xt, LEVELS)
    assert results[0][:3] == (hw.tolist(), m, n_nan)
    cal = Calibration.from_select(LEVELS, (hw, m, n_nan))
    assert results[0][3] == loadtest.coverage_metrics(cal, 1.0 + 0.5 * Xt, yt)
