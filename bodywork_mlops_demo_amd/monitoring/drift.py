"""Distribution-level drift monitoring: PSI / KS on fused device histograms.

The scalar metric CSVs cannot see the generator's drift: labels reach down
to zero (the ``y >= 0`` cull), so ``|score/label - 1|`` is heavy-tailed and
the online/offline MAPE ratio is seed noise.  The residual distribution
``label - score`` follows the drifting intercept monotonically, so this
module compares binned distributions instead:

- :class:`HistSpec` fixes the bins; :func:`ops.drift_histograms` counts
  ``X``, ``labels``, ``scores`` and the residual in one pass over the
  tensors stage 4 already holds.
- :func:`psi`, :func:`ks`, :func:`js`, :func:`quantile` and
  :func:`ks_critical` are pure numpy on count vectors.
- :class:`DriftMonitor` keeps a reference (the newest training day scored
  by the freshly trained model) and turns each observed day into the
  statistics and one decision, ``drifted``.

Cells: a histogram row is ``[under, bin_1 .. bin_B, over, nan]``.  The
under / over cells take part in every statistic as ordinary cells.  The NaN
cell has no place on the axis: it is one more category for PSI and is left
out of the ordered statistics (KS, quantiles) and of their sample sizes.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np
import torch

from bodywork_mlops_demo_amd import ops

ROWS = ("x", "label", "score", "residual")


@dataclass(frozen=True)
class HistSpec:
    """``bins`` equal cells over ``[lo, hi)`` per histogram row; the
    defaults suit the generator (X ~ U(0, 100), y ~ 1 + 0.5 X + 10 eps).
    Anything outside a range lands in that row's under / over cell."""

    bins: int = 64
    x: tuple = (0, 100)
    label: tuple = (0, 128)
    score: tuple = (0, 128)
    residual: tuple = (-50, 50)

    def __post_init__(self):
        if not 1 <= int(self.bins) <= 256:
            raise ValueError(f"HistSpec: 1 <= bins <= 256 (got {self.bins})")
        for name, (lo, hi) in zip(ROWS, self.ranges()):
            if not np.float32(hi) > np.float32(lo):
                raise ValueError(f"HistSpec: empty range for {name}: "
                                 f"({lo}, {hi})")

    def ranges(self) -> list[tuple]:
        return [tuple(self.x), tuple(self.label), tuple(self.score),
                tuple(self.residual)]

    def bin_params(self) -> tuple[list[float], list[float]]:
        """``(lo, scale)`` per row as fp32 values (held in Python floats):
        ``scale = fp32(bins) / (fp32(hi) - fp32(lo))``.  The only place
        the scale is computed; the kernel and the oracle take it as given."""
        lo = [np.float32(r[0]) for r in self.ranges()]
        scale = [np.float32(self.bins) / (np.float32(r[1]) - l)
                 for r, l in zip(self.ranges(), lo)]
        return [float(v) for v in lo], [float(v) for v in scale]


# --------------------------------------------------------------------------
# statistics on count vectors
# --------------------------------------------------------------------------

def _counts(c) -> np.ndarray:
    return np.asarray(c, dtype=np.float64).reshape(-1)


def psi(ref, cur, eps: float = 0.5) -> float:
    """Population stability index ``sum (q - p) ln(q / p)`` over the cells,
    with additive smoothing: ``p = (ref + eps) / (sum(ref) + eps * K)``.
    Symmetric in its arguments."""
    r, c = _counts(ref), _counts(cur)
    k = r.shape[0]
    p = (r + eps) / (r.sum() + eps * k)
    q = (c + eps) / (c.sum() + eps * k)
    return float(np.sum((q - p) * np.log(q / p)))


def _cdf(c: np.ndarray) -> np.ndarray:
    tot = c.sum()
    return np.cumsum(c) / tot if tot > 0 else np.zeros_like(c)


def ks(ref, cur) -> float:
    """Largest absolute gap between the two binned CDFs.  Never above the
    KS distance of the unbinned samples."""
    return float(np.max(np.abs(_cdf(_counts(ref)) - _cdf(_counts(cur)))))


def js(ref, cur) -> float:
    """Jensen-Shannon divergence of the two cell distributions (natural
    log: 0 for equal, ln 2 for disjoint)."""
    r, c = _counts(ref), _counts(cur)
    p = r / r.sum() if r.sum() > 0 else r
    q = c / c.sum() if c.sum() > 0 else c
    m = 0.5 * (p + q)

    def kl(a):
        nz = a > 0
        return float(np.sum(a[nz] * np.log(a[nz] / m[nz])))

    return 0.5 * kl(p) + 0.5 * kl(q)


def quantile(counts, spec_range, q: float) -> float:
    """The ``q``-quantile of ``counts = [under, bin_1 .. bin_B, over]``
    over ``spec_range = (lo, hi)``, linear inside a bin.  A quantile that
    falls into the under / over cell is ``lo`` / ``hi``."""
    c = _counts(counts)
    lo, hi = float(spec_range[0]), float(spec_range[1])
    bins = c.shape[0] - 2
    tot = c.sum()
    if tot <= 0:
        return float("nan")
    target = q * tot
    cum = np.cumsum(c)
    i = int(np.searchsorted(cum, target, side="left"))
    i = min(i, c.shape[0] - 1)
    if i == 0:
        return lo
    if i == bins + 1:
        return hi
    frac = (target - cum[i - 1]) / c[i]
    return float(lo + (i - 1 + frac) * (hi - lo) / bins)


def ks_critical(n_ref: float, n_cur: float, alpha: float = 1e-3) -> float:
    """Two-sample Kolmogorov-Smirnov critical value at level ``alpha``:
    ``sqrt(-ln(alpha / 2) / 2) * sqrt((n_ref + n_cur) / (n_ref * n_cur))``.
    Binned KS never exceeds the true KS, so testing it against this value
    is conservative."""
    if n_ref <= 0 or n_cur <= 0:
        return float("inf")
    return (math.sqrt(-math.log(alpha / 2.0) / 2.0)
            * math.sqrt((n_ref + n_cur) / (n_ref * n_cur)))


# --------------------------------------------------------------------------
# the monitor
# --------------------------------------------------------------------------

class DriftMonitor:
    """Reference histograms + per-day statistics and the ``drifted``
    decision: ``ks_residual > max(ks_critical, ks_threshold or 0)``.

    With a ``process_group`` the int64 counts are all-reduced (SUM) before
    any statistic, so every rank gets the same numbers and the same
    decision."""

    def __init__(self, spec: HistSpec | None = None, alpha: float = 1e-3,
                 ks_threshold: float | None = None, process_group=None):
        self.spec = spec or HistSpec()
        self.alpha = alpha
        self.ks_threshold = ks_threshold
        self.process_group = process_group
        self.reference: np.ndarray | None = None

    def histograms(self, X: torch.Tensor, labels: torch.Tensor,
                   scores: torch.Tensor) -> np.ndarray:
        """int64 ``[4, bins + 3]`` counts (summed over the process group)."""
        h = ops.drift_histograms(X, labels, scores, self.spec)
        if self.process_group is not None:
            import torch.distributed as dist

            if dist.get_backend(self.process_group) != "nccl":
                h = h.cpu()
            dist.all_reduce(h, op=dist.ReduceOp.SUM, group=self.process_group)
        return h.cpu().numpy()

    def set_reference(self, X: torch.Tensor, labels: torch.Tensor,
                      scores: torch.Tensor) -> None:
        self.reference = self.histograms(X, labels, scores)

    def observe(self, X: torch.Tensor, labels: torch.Tensor,
                scores: torch.Tensor) -> dict:
        if self.reference is None:
            raise RuntimeError("DriftMonitor.observe before set_reference")
        return self.statistics(self.reference,
                               self.histograms(X, labels, scores))

    def statistics(self, ref: np.ndarray, cur: np.ndarray) -> dict:
        """The ``observe`` dict from two ``[4, bins + 3]`` count arrays."""
        out = {f"psi_{name}": psi(ref[k], cur[k])
               for k, name in enumerate(ROWS)}
        r, c = ref[3, :-1], cur[3, :-1]  # residual row, ordered cells
        out["ks_residual"] = ks(r, c)
        out["ks_critical"] = ks_critical(float(r.sum()), float(c.sum()),
                                         self.alpha)
        for q, key in ((0.05, "q05"), (0.5, "q50"), (0.95, "q95")):
            out[f"residual_{key}"] = quantile(c, self.spec.residual, q)
        out["drifted"] = bool(
            out["ks_residual"] > max(out["ks_critical"],
                                     self.ks_threshold or 0.0))
        return out


#: the columns `observe` adds to a test-metrics CSV row, in order
METRIC_KEYS = ("psi_x", "psi_label", "psi_score", "psi_residual",
               "ks_residual", "ks_critical", "residual_q05", "residual_q50",
               "residual_q95", "drifted")
