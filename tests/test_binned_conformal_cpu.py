"""x-dependent conformal intervals off the GPU: the CPU op against a plain
per-cell sort, the binned calibration's dict round trip, the service's
per-row widths and what ``train(conformal_bins=...)`` stores."""
from datetime import date

import numpy as np
import pytest
import torch

from bodywork_mlops_demo_amd import ops
from bodywork_mlops_demo_amd.models.conformal import Calibration, Cells
from bodywork_mlops_demo_amd.stages import datagen, loadtest, train


@pytest.fixture()
def seeded_store(tmp_store):
    for day in (1, 2, 3):
        datagen.run(tmp_store, n=800, date=date(2026, 1, day), device="cpu",
                    seed=day)
    return tmp_store


@pytest.mark.parametrize("cells", [1, 3, 16])
def test_cpu_op_is_a_per_cell_sort(cells):
    rng = np.random.default_rng(7)
    n, levels, g = 5003, (0.5, 0.9, 0.999), Cells(cells)
    x = rng.uniform(-10, 110, n).astype(np.float32)
    lab = rng.normal(0, 10, n).astype(np.float32)
    lab[::97], x[::211] = np.nan, np.nan
    s = np.zeros(n, dtype=np.float32)
    hw, m, n_nan = ops.binned_residual_quantiles(
        torch.from_numpy(x), torch.from_numpy(lab), torch.from_numpy(s),
        levels, g)
    # the rule written out: scale, clamp, truncate, in float32
    t = (x - np.float32(0)) * (np.float32(cells) / np.float32(100))
    cell = np.clip(np.nan_to_num(t, nan=0.0), 0, cells - 1).astype(np.int64)
    cell[np.isnan(x)] = -1
    assert (g.cell_of(x) == cell).all()
    assert n_nan == np.count_nonzero(np.isnan(x) | np.isnan(lab))
    for c in range(cells):
        v = np.sort(np.abs(lab[(cell == c) & ~np.isnan(lab)]))
        assert m[c] == v.size
        for q, L in enumerate(levels):
            k = int(np.ceil((v.size + 1) * L))
            assert hw[c, q].item() == (v[k - 1] if k <= v.size else np.inf)
    cov = ops.binned_interval_coverage(
        torch.from_numpy(x), torch.from_numpy(s), torch.from_numpy(lab), hw, g)
    assert cov[:, 0].tolist() == m.tolist()
    assert (cov[:, 1:4] >= torch.ceil((m[:, None] + 1) * torch.tensor(levels))
            .clamp(max=m[:, None])).all() and (cov[:, 4] == 0).all()


def test_calibration_dict_round_trip():
    plain = Calibration((0.9,), (15.5,), 100, 1, "2026-01-03")
    assert set(plain.as_dict()) == {"levels", "halfwidths", "m", "n_nan",
                                    "date"}
    cal = plain.with_cells(Cells(2, 0, 50), (
        torch.tensor([[11.5], [16.25]]), torch.tensor([40, 60]), 1))
    d = cal.as_dict()
    assert d["cells"] == [2, 0.0, 50.0] and d["cell_m"] == [40, 60]
    assert d["cell_halfwidths"] == [[11.5], [16.25]]
    assert Calibration.from_dict(d) == cal
    assert Calibration.from_dict(plain.as_dict()) == plain
    assert cal.halfwidth(0.9) == 15.5
    assert cal.halfwidth_at(0.9, [10.0, 30.0, float("nan")]).tolist() == \
        [11.5, 16.25, 15.5]
    with pytest.raises(ValueError):
        Cells(17)
    with pytest.raises(ValueError):
        Cells(4, 5.0, 5.0)


def test_train_stores_what_the_op_returns_and_the_service_serves_it(
        seeded_store):
    from fastapi.testclient import TestClient

    from bodywork_mlops_demo_amd.serving.server import create_app

    with pytest.raises(ValueError):
        train.run(seeded_store, device="cpu", conformal_bins=4)
    _, model = train.run(seeded_store, model_type="linear", device="cpu",
                         conformal_levels=(0.9,), conformal_bins=4,
                         return_model=True)
    cal = model.conformal_
    y_np, X_np, _ = seeded_store.get_all_datasets()
    _, _, X_te, y_te = ops.random_split(torch.from_numpy(X_np),
                                        torch.from_numpy(y_np), 0.2, seed=42)
    hw, m, _ = ops.binned_residual_quantiles(X_te, y_te, model.predict(X_te),
                                             (0.9,), Cells(4))
    assert cal.cells == Cells(4) and list(cal.cell_m) == m.tolist()
    assert [list(r) for r in cal.cell_halfwidths] == hw.tolist()
    assert cal.halfwidths == tuple(ops.residual_quantiles(
        y_te, model.predict(X_te), (0.9,))[0].tolist())
    assert seeded_store.get_latest_model()[0].conformal_ == cal.as_dict()
    widths = [r[0] for r in cal.cell_halfwidths]
    assert widths[0] != widths[3]

    with TestClient(create_app(seeded_store, device="cpu")) as client:
        def width(x):
            lo, hi = client.post(
                "/score/v1", json={"X": x, "confidence": 0.9}).json()["interval"]
            return (hi - lo) / 2
        for x, c in ((5, 0), (80, 3), (-5, 0), (1e6, 3)):
            assert width(x) == pytest.approx(widths[c], rel=1e-5)
        batch = client.post("/score/v1/batch",
                            json={"X": [5, 80], "confidence": 0.9}).json()
        (lo0, hi0), (lo1, hi1) = batch["interval"]
        assert hi0 - lo0 != hi1 - lo1
        r = client.post("/score/v1/binary",
                        content=np.float32([5, 80]).tobytes())
        assert r.headers["X-Interval-Cells"] == "4,0.0,100.0"
        assert [float(v) for v in
                r.headers["X-Interval-Cell-Halfwidths"].split(",")] == widths

    # stage 4 checks the x-dependent band, overall and per cell
    labels, X = torch.from_numpy(y_np), torch.from_numpy(X_np)
    on = loadtest.coverage_metrics(cal, model.predict(X), labels, X=X)
    counts = ops.binned_interval_coverage(X, model.predict(X), labels,
                                          cal.cell_halfwidths, cal.cells)
    assert on["pi90_cell_coverage"] == [c / n for n, c in
                                        counts[:, :2].tolist()]
    assert on["pi90_coverage"] == counts[:, 1].sum().item() / counts[:, 0].sum().item()
    assert on["pi90_worst_cell_coverage"] == min(on["pi90_cell_coverage"])
    assert on["pi90_ok"] == on["pi90_cells_ok"] == 1
