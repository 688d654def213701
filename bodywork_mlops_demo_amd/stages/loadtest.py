"""stage-4-test-model-scoring-service: load-test the live service.

Reference semantics (``stage_4_test_model_scoring_service.py:31-36``):
download the latest (t+1) dataset, score every row against the live
stage-2 service, time each request (3 retries, -1 sentinels on failure),
compute live metrics (MAPE = mean |score/label - 1|, score-label
correlation, max APE, mean response time) and persist the test-metrics
CSV.

Client modes:
- ``serial``  — reference parity: one POST per row, new session per call
  (``stage_4:68-85``); the reference's own throughput profile.
- ``batch``   — the MI355X client: rows are scored in large chunks
  against ``/score/v1/batch`` so one request drives one fused
  (hipGraph-replayed) GPU launch; ``response_time`` is per-chunk wall
  time, amortised per row.  This is the rows/sec headline path.

Metric computation itself runs as one fused GPU reduction when a device
is available (``ops.score_label_metrics``).
"""
from __future__ import annotations

import argparse
from datetime import date as date_t
from time import perf_counter

import numpy as np
import torch

from bodywork_mlops_demo_amd import ops
from bodywork_mlops_demo_amd.monitoring import stage_guard
from bodywork_mlops_demo_amd.store import ArtefactStore, contract, open_store
from bodywork_mlops_demo_amd.utils.logging import configure_logger

log = configure_logger(__name__)

STAGE_NAME = "stage-4-test-model-scoring-service"
DEFAULT_URL = "http://127.0.0.1:5000/score/v1"


def _score_serial(url: str, X: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """Reference-parity serial client (stage_4:66-98)."""
    import requests
    from requests.exceptions import ConnectionError, Timeout

    scores = np.empty(X.shape[0])
    times = np.empty(X.shape[0])
    for i, x in enumerate(X):
        session = requests.Session()
        session.mount(url, requests.adapters.HTTPAdapter(max_retries=3))
        t0 = perf_counter()
        try:
            resp = session.post(url, json={"X": float(x)}, timeout=30)
            times[i] = perf_counter() - t0
            scores[i] = resp.json()["prediction"] if resp.ok else -1
        except (ConnectionError, Timeout) as e:
            log.error(e)
            scores[i], times[i] = -1, -1
    return scores, times


def _urls(url: str | list[str]) -> list[str]:
    """Resolve the replica URL set: an explicit list, a comma-separated
    env value (the runner's service-discovery channel, standing in for
    the k8s ClusterIP load balancer), or the single URL given."""
    if isinstance(url, list):
        return url
    if "," in url:
        return [u.strip() for u in url.split(",") if u.strip()]
    return [url]


def _score_batch(
    url: str | list[str], X: np.ndarray, chunk: int = 65536
) -> tuple[np.ndarray, np.ndarray]:
    """Chunked batch client against /score/v1/batch, chunks round-robined
    across serving replicas."""
    import requests

    urls = [u.rstrip("/") + ("" if u.endswith("/batch") else "/batch")
            for u in _urls(url)]
    session = requests.Session()
    for u in urls:
        session.mount(u, requests.adapters.HTTPAdapter(max_retries=3))
    scores = np.empty(X.shape[0])
    times = np.empty(X.shape[0])
    for ci, lo in enumerate(range(0, X.shape[0], chunk)):
        hi = min(lo + chunk, X.shape[0])
        t0 = perf_counter()
        resp = session.post(
            urls[ci % len(urls)],
            json={"X": [float(v) for v in X[lo:hi]]}, timeout=300,
        )
        dt = perf_counter() - t0
        if resp.ok:
            scores[lo:hi] = np.asarray(resp.json()["predictions"])
        else:
            scores[lo:hi] = -1
        times[lo:hi] = dt / (hi - lo)
    return scores, times


def _score_binary(
    url: str | list[str], X: np.ndarray, chunk: int = 1 << 20
) -> tuple[np.ndarray, np.ndarray]:
    """Binary batch client (raw float32 in/out), round-robined across
    replicas; with >1 replica the chunks go out concurrently (one worker
    per replica — the shared-nothing GPU fan-out)."""
    import requests

    urls = [u.rstrip("/") + "/binary" for u in _urls(url)]
    session = requests.Session()
    for u in urls:
        session.mount(u, requests.adapters.HTTPAdapter(max_retries=3))
    scores = np.empty(X.shape[0], dtype=np.float32)
    times = np.empty(X.shape[0])

    def _one(ci: int, lo: int, hi: int):
        t0 = perf_counter()
        resp = session.post(
            urls[ci % len(urls)], data=X[lo:hi].astype(np.float32).tobytes(),
            headers={"Content-Type": "application/octet-stream"}, timeout=300,
        )
        dt = perf_counter() - t0
        if resp.ok:
            scores[lo:hi] = np.frombuffer(resp.content, dtype=np.float32)
        else:
            scores[lo:hi] = -1
        times[lo:hi] = dt / (hi - lo)

    chunks = [(ci, lo, min(lo + chunk, X.shape[0]))
              for ci, lo in enumerate(range(0, X.shape[0], chunk))]
    if len(urls) > 1:
        from concurrent.futures import ThreadPoolExecutor

        with ThreadPoolExecutor(len(urls)) as pool:
            list(pool.map(lambda c: _one(*c), chunks))
    else:
        for c in chunks:
            _one(*c)
    return scores, times


#: one-sided 1e-3 normal quantile of the coverage check (the level of
#: ``ks_alpha``'s default)
COVERAGE_Z = 3.09


def _calibration(conformal, store):
    """``conformal`` as a Calibration: itself, or (``True``) the one on the
    latest model artefact."""
    from bodywork_mlops_demo_amd.models.conformal import Calibration, restore

    if isinstance(conformal, Calibration):
        return conformal
    artefact, _ = store.get_latest_model()
    cal = restore(artefact)
    if cal is None:
        raise ValueError("the latest model artefact carries no conformal "
                         "calibration (train with conformal levels)")
    return cal


def coverage_metrics(cal, scores: torch.Tensor, labels: torch.Tensor,
                     process_group=None) -> dict:
    """``pi<pct>_coverage`` / ``_halfwidth`` / ``_ok`` per level of ``cal``,
    in that order level by level, from one coverage pass."""
    from bodywork_mlops_demo_amd.models.conformal import level_name

    counts = ops.interval_coverage(scores, labels, cal.halfwidths)
    if process_group is not None:
        counts = ops.allreduce_counts(counts, process_group)
    counts = counts.tolist()
    n = counts[0]
    out = {}
    for q, (level, h) in enumerate(zip(cal.levels, cal.halfwidths)):
        pct = level_name(level)
        coverage = counts[1 + q] / n if n > 0 else float("nan")
        floor = level - COVERAGE_Z * (level * (1.0 - level) / n) ** 0.5 \
            if n > 0 else 0.0
        out[f"pi{pct}_coverage"] = coverage
        out[f"pi{pct}_halfwidth"] = h
        out[f"pi{pct}_ok"] = 0 if coverage < floor else 1
    return out


def run(
    store: ArtefactStore,
    url: str = DEFAULT_URL,
    mode: str = "batch",
    device: str | None = None,
    scorer=None,
    data: tuple[torch.Tensor, torch.Tensor, date_t] | None = None,
    persist: bool = True,
    capture: dict | None = None,
    drift_monitor=None,
    conformal=None,
    process_group=None,
) -> dict:
    """Score the latest dataset against the service; persist test metrics.

    ``drift_monitor`` (a :class:`monitoring.drift.DriftMonitor` with its
    reference set) observes the tensors held here; its statistics join the
    returned metrics and are appended as columns to the test-metrics CSV.
    Without one the metrics and the CSV are unchanged.

    ``conformal`` (a :class:`models.conformal.Calibration`, or ``True``:
    read it from the latest model artefact) checks the deployed model's
    prediction intervals on the rows held here, in one
    ``ops.interval_coverage`` pass: per level the metrics and the CSV gain
    ``pi<pct>_coverage``, ``pi<pct>_halfwidth`` and ``pi<pct>_ok`` — 1
    unless the coverage falls below ``level - z * sqrt(level * (1 - level)
    / n)`` with z = 3.09, a one-sided 1e-3 binomial test.  These columns
    come last.  With a ``process_group`` the counts are all-reduced.

    ``scorer`` bypasses HTTP entirely (in-process serving replica) for the
    hermetic pipeline/bench path; ``data`` skips the store read when the
    tensors are already device-resident.  ``capture``, when given, receives
    references to the tensors the metrics were computed from (``X``,
    ``labels``, ``scores``) — no extra work, the caller just gets to see them.
    """
    device = device or ("cuda" if torch.cuda.is_available() else "cpu")
    if data is None:
        key, data_date = store.latest(contract.DATASETS_PREFIX)
        y_np, X_np = store.get_dataset(key)
        labels = torch.from_numpy(y_np)
        X = torch.from_numpy(X_np)
    else:
        labels, X, data_date = data

    n = X.shape[0]
    if scorer is not None:
        # in-process replica: no HTTP on this path, so the per-row time is
        # an AMORTISED GPU batch time, not a response latency — the kind
        # column below says so in the persisted artefact
        rt_kind = "amortised-gpu-batch"
        t0 = perf_counter()
        scores_t = scorer.score_tensor(X.to(device))
        if device.startswith("cuda"):
            # this stream only: an artefact D2H in flight on another
            # stream is not part of the scoring time
            torch.cuda.current_stream(torch.device(device)).synchronize()
        mean_rt = (perf_counter() - t0) / n
        scores = scores_t
    else:
        rt_kind = f"http-{mode}"
        X_np = X.cpu().numpy()
        if mode == "serial":
            scores_np, times = _score_serial(url, X_np)
        elif mode == "batch":
            scores_np, times = _score_batch(url, X_np)
        elif mode == "binary":
            scores_np, times = _score_binary(url, X_np)
        else:
            raise ValueError(f"unknown client mode {mode!r}")
        mean_rt = float(times.mean())
        scores = torch.from_numpy(scores_np.astype(np.float32))

    scores = scores.to(device)
    labels = labels.to(device)
    if capture is not None:
        capture.update(X=X, labels=labels, scores=scores)
    metrics = ops.score_label_metrics(scores, labels)
    metrics["mean_response_time"] = mean_rt
    metrics["response_time_kind"] = rt_kind
    metrics["rows_per_sec"] = n / (mean_rt * n) if mean_rt > 0 else float("inf")
    drift_keys: tuple = ()
    if drift_monitor is not None:
        from bodywork_mlops_demo_amd.monitoring.drift import METRIC_KEYS

        metrics.update(drift_monitor.observe(X.to(device), labels, scores))
        drift_keys = METRIC_KEYS
    pi_keys: tuple = ()
    if conformal:
        cal = _calibration(conformal, store)
        cov = coverage_metrics(cal, scores, labels, process_group)
        metrics.update(cov)
        pi_keys = tuple(cov)
    log.info(f"live-service metrics on {n} rows: {metrics}")

    if persist:
        key = contract.test_metrics_key(data_date)
        # reference schema (stage_4:106-112) + a kind column so the
        # amortised in-process figure can never be read as a latency;
        # the drift monitor's columns, when there is one, come last
        store.put_metrics_csv(
            key,
            ["date", "MAPE", "r_squared", "max_residual",
             "mean_response_time", "response_time_kind", *drift_keys,
             *pi_keys],
            [data_date, metrics["MAPE"], metrics["r_squared"],
             metrics["max_residual"], metrics["mean_response_time"],
             rt_kind,
             # the decision as 0/1 so the analytics read it as a number
             *(int(metrics[k]) if k == "drifted" else metrics[k]
               for k in drift_keys),
             *(metrics[k] for k in pi_keys)],
        )
        log.info(f"uploaded test metrics to {key}")
    return metrics


def main(argv=None) -> None:
    import os

    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument("--store", default=None)
    p.add_argument(
        "--url",
        default=os.environ.get(
            "BODYWORK_AMD_SERVICE_URLS",  # all replicas (comma-separated)
            os.environ.get("BODYWORK_AMD_SERVICE_URL", DEFAULT_URL),
        ),
    )
    p.add_argument("--mode", default="batch",
                   choices=["serial", "batch", "binary"])
    p.add_argument("--device", default=None)
    p.add_argument("--conformal", action="store_true",
                   default=bool(os.environ.get("BODYWORK_AMD_CONFORMAL")),
                   help="check the coverage of the prediction intervals the "
                        "latest model artefact was calibrated for (default: "
                        "on when $BODYWORK_AMD_CONFORMAL is set)")
    args = p.parse_args(argv)
    with stage_guard(STAGE_NAME, exit_on_error=True):
        run(open_store(args.store), url=args.url, mode=args.mode,
            device=args.device, conformal=args.conformal or None)


if __name__ == "__main__":
    main()
