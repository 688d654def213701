"""stage-1-train-model: fit a regressor on all accumulated data.

Reference semantics (``stage_1_train_model.py:31-36``): download every
dataset in time order, 80/20 split with seed 42, fit, compute offline
metrics (MAPE / R^2 / max residual), persist joblib model + metrics CSV
keyed by the newest dataset date.

MI355X path: datasets load into HBM once, the OLS fit is one fused HIP
statistics reduction (or MFMA GEMM training steps for the MLP config),
and in DP mode each rank holds a row shard with RCCL all-reduce of the
statistics/gradients.
"""
from __future__ import annotations

import argparse
import os
from datetime import date as date_t

import torch

from bodywork_mlops_demo_amd import ops
from bodywork_mlops_demo_amd.models import (
    GPULinearRegressor,
    GPUMLPRegressor,
    GPUPolyRegressor,
    GPUPolyRegressorCV,
)
from bodywork_mlops_demo_amd.models.conformal import Calibration, level_name
from bodywork_mlops_demo_amd.monitoring import stage_guard
from bodywork_mlops_demo_amd.store import ArtefactStore, contract, open_store
from bodywork_mlops_demo_amd.utils.logging import configure_logger

log = configure_logger(__name__)

STAGE_NAME = "stage-1-train-model"


def default_device() -> str:
    return "cuda" if torch.cuda.is_available() else "cpu"


def run(
    store: ArtefactStore,
    model_type: str = "linear",
    device: str | None = None,
    process_group=None,
    rank: int = 0,
    world_size: int = 1,
    mlp_steps: int = 50,
    mlp_batch_size: int = 65536,
    data: tuple[torch.Tensor, torch.Tensor, date_t] | None = None,
    return_model: bool = False,
    model_cache: dict | None = None,
    conformal_levels=None,
):
    """Train and persist; returns the offline metrics record
    (or ``(metrics, model)`` when ``return_model``).

    ``data`` short-circuits store reads when the caller already holds the
    tensors in HBM (the in-process pipeline keeps data resident instead of
    re-reading artefacts — SURVEY.md §7 'keep tensors resident').

    ``conformal_levels`` (up to four confidence levels in (0, 1)) calibrates
    split-conformal prediction intervals on the 20 % hold-out: the
    half-widths go onto the model (``conformal_``, and into its artefact)
    and are appended to the model-metrics CSV as ``pi_cal_n`` and one
    ``pi<pct>_halfwidth`` per level.  Without levels neither changes.
    """
    device = device or default_device()
    levels = (ops.check_levels(conformal_levels)
              if conformal_levels is not None else None)
    if data is None:
        y_np, X_np, data_date = store.get_all_datasets()
        X = torch.from_numpy(X_np).to(device)
        y = torch.from_numpy(y_np).to(device)
    else:
        y, X, data_date = data
        X, y = X.to(device), y.to(device)

    if world_size > 1:  # row-shard for DP
        X, y = X[rank::world_size], y[rank::world_size]

    n = X.shape[0]
    log.info(f"training {model_type} regressor on {n} rows (device={device})")
    # on-device philox split (reference: 80/20, seed 42 —
    # stage_1:98-103); count is binomial(n, 0.2) rather than exactly n/5
    metrics = None
    if model_type != "linear":
        X_train, y_train, X_test, y_test = ops.random_split(X, y, 0.2,
                                                            seed=42)

    if model_type == "linear":
        # the linear fit and its offline metrics are two streaming
        # reductions, so the same split is evaluated inside them instead
        # of being scattered into four arrays that are each read once
        model = GPULinearRegressor(device=device)
        metrics = model.fit_split(X, y, 0.2, seed=42,
                                  process_group=process_group)
    elif model_type.startswith("polycv"):
        # "polycv" (degrees 1..5) or "polycv<d>" (degrees 1..d): degree
        # and l2 chosen by K-fold CV from one fold-statistics pass
        max_degree = int(model_type[6:]) if len(model_type) > 6 else 5
        model = GPUPolyRegressorCV(max_degree=max_degree, device=device).fit(
            X_train, y_train, process_group=process_group
        )
    elif model_type.startswith("poly"):
        # "poly" (degree 3) or "poly<d>", e.g. "poly2"
        degree = int(model_type[4:]) if len(model_type) > 4 else 3
        model = GPUPolyRegressor(degree=degree, device=device).fit(
            X_train, y_train, process_group=process_group
        )
    elif model_type == "mlp":
        # reuse the cached model object so its captured training graph
        # survives across daily retrains (weights re-randomised in place).
        # The same date-derived seed feeds both the warm (reinit_) and
        # cold (constructor) paths, and both draw the same CPU generator
        # stream — the day's initial weights are identical regardless of
        # cache warmth or process restarts.
        init_seed = 7 + data_date.toordinal()
        model = None
        if model_cache is not None:
            cached = model_cache.get("mlp")
            if (isinstance(cached, GPUMLPRegressor)
                    and str(cached.device) == str(torch.device(device))):
                model = cached.reinit_(seed=init_seed)
        if model is None:
            model = GPUMLPRegressor(device=device, seed=init_seed)
            if model_cache is not None:
                model_cache["mlp"] = model
        model.fit(
            X_train, y_train, steps=mlp_steps, batch_size=mlp_batch_size,
            process_group=process_group,
        )
    else:
        raise ValueError(f"unknown model_type {model_type!r}")

    yhat = None
    if metrics is None:
        yhat = model.predict(X_test)
        metrics = ops.regression_metrics(y_test, yhat)
    log.info(f"offline metrics: {metrics}")

    model.conformal_ = None
    if levels is not None:
        if model_type == "linear":
            # the same never-materialised split as the fit: flag and score
            # are evaluated inside the select passes
            on_dev = X.device.type == "cuda" and model.device.type == "cuda"
            ab = (model._ab_tensor() if on_dev
                  else (model.intercept_, model.coef_))
            selected = ops.linear_split_residual_quantiles(
                X, y, ab, levels, 0.2, seed=42, process_group=process_group)
        else:
            selected = ops.residual_quantiles(
                y_test, yhat, levels, process_group=process_group)
        model.conformal_ = Calibration.from_select(levels, selected,
                                                   date=data_date)
        log.info(f"conformal calibration: {model.conformal_}")

    if rank == 0:
        model_key = store.put_model(model.to_sklearn(), data_date)
        log.info(f"uploaded model to {model_key}")
        metrics_key = contract.model_metrics_key(data_date)
        header = ["date", "MAPE", "r_squared", "max_residual"]
        row = [data_date, metrics["MAPE"], metrics["r_squared"],
               metrics["max_residual"]]
        if isinstance(model, GPUPolyRegressorCV):
            # what the cross-validation chose; this model type only
            header += ["cv_degree", "cv_l2", "cv_mse", "cv_folds"]
            row += [model.degree, model.l2, model.best_score_, model.folds]
        if model.conformal_ is not None:
            cal = model.conformal_
            header += ["pi_cal_n"] + [f"pi{level_name(lv)}_halfwidth"
                                      for lv in cal.levels]
            row += [cal.m, *cal.halfwidths]
        store.put_metrics_csv(metrics_key, header, row)
        log.info(f"uploaded metrics to {metrics_key}")
    if return_model:
        return metrics, model
    return metrics


def parse_levels(text: str) -> tuple[float, ...]:
    """``"0.9,0.95"`` -> ``(0.9, 0.95)`` for the ``--conformal`` options."""
    try:
        return ops.check_levels(float(v) for v in text.split(",") if v.strip())
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e)) from e


def main(argv=None) -> None:
    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument("--store", default=None, help="store URI (dir or s3://bucket)")
    p.add_argument("--model", default="linear",
                   help="linear | poly[<degree>] | polycv[<max degree>] "
                        "(degree and l2 by 5-fold CV) | mlp")
    p.add_argument("--device", default=None)
    p.add_argument("--mlp-steps", type=int, default=50)
    p.add_argument("--conformal", type=parse_levels, metavar="LEVELS",
                   default=os.environ.get("BODYWORK_AMD_CONFORMAL") or None,
                   help="calibrate prediction intervals at these confidence "
                        "levels, e.g. 0.9,0.95 (at most 4, each in (0, 1)); "
                        "default: $BODYWORK_AMD_CONFORMAL")
    args = p.parse_args(argv)
    with stage_guard(STAGE_NAME, exit_on_error=True):
        run(open_store(args.store), model_type=args.model, device=args.device,
            mlp_steps=args.mlp_steps, conformal_levels=args.conformal)


if __name__ == "__main__":
    main()
